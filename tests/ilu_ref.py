"""A plain numpy / Python restatement of the contract of g4s_ilu0_* (include/g4s.h): which matrices are refused and with which row, the row-wise ILU(0)
loop in the documented arithmetic — per k ascending the quotient w_p / u_kk, then w_t − (w_p · u_kj) at the stored positions, product and difference
rounded separately —, the canonical NaN of a finished row, bad_pivot, and the info fields. The levels and the launch plan are those of the strictly lower
triangle (tests/trsv_ref.py: levels, launch_plan), the apply is two of its solves. test_ilu_cpu.py pins it to dense LU, to exact rationals and to
(L U)_ij = a_ij on the pattern; test_ilu_gpu.py compares the device with it bit for bit. The cases are built once and shared; nobody writes to them."""
import functools

import numpy as np

from tests import trsv_ref as tr

LANE_ROW, WAVE_ROW = 8, 512
CHAIN_WIDTH, CHAIN_LEVELS = tr.CHAIN_WIDTH, tr.CHAIN_LEVELS
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def refusal(n, rp, ci):
    """None for a matrix the analysis takes; ("rowptr", −1) for a rowptr that does not start at 0 or decreases; else (kind, row) of the smallest row
    that stores an id outside [0, n) ("id"), or whose ids do not ascend strictly ("order"), or that stores no diagonal entry ("diag") — per row the
    first of the three that applies"""
    rp = np.asarray(rp, np.int64)
    if n and (rp[0] != 0 or np.any(np.diff(rp) < 0)):
        return "rowptr", -1
    for i in range(n):
        c = np.asarray(ci[rp[i]:rp[i + 1]], np.int64)
        if np.any((c < 0) | (c >= n)):
            return "id", i
        if np.any(np.diff(c) <= 0):
            return "order", i
        if i not in c:
            return "diag", i
    return None


REFUSAL_TEXT = {"rowptr": "rowptr must start at 0 and never decrease", "id": "stores a column id outside [0, n)", "order": "is not strictly ascending",
                "diag": "stores no diagonal entry"}


def factor(n, rp, ci, va):
    """(f, bad_pivot): f in the layout of va — L strictly below the diagonal (unit diagonal implied), U on and above it"""
    f = np.array(va, np.float64)
    dpos = np.zeros(n, np.int64)
    bad = -1
    with np.errstate(all="ignore"):
        for i in range(n):
            rb, re = int(rp[i]), int(rp[i + 1])
            pos = {int(ci[q]): q for q in range(rb, re)}
            dpos[i] = pos[i]
            for p in range(rb, re):
                k = int(ci[p])
                if k >= i:
                    break
                wp = f[p] / f[dpos[k]]
                f[p] = wp
                for q in range(int(dpos[k]) + 1, int(rp[k + 1])):
                    t = pos.get(int(ci[q]))
                    if t is not None:
                        prod = wp * f[q]
                        f[t] = f[t] - prod
            row = f[rb:re]
            row[np.isnan(row)] = QNAN
            u = f[dpos[i]]
            if bad < 0 and (u == 0.0 or not np.isfinite(u)):
                bad = i
    return f, bad


def apply(n, rp, ci, f, r):
    """z = U⁻¹ (L⁻¹ r): the lower unit solve and the upper solve of trsv_ref on the factor array"""
    return tr.solve(n, rp, ci, f, tr.solve(n, rp, ci, f, r, True, True), False, False)


def info(n, rp, ci, va, no_chains=False):
    """the fields of g4s_ilu0_info that are a function of the matrix and the flag"""
    low = tr.info(n, rp, ci, va, True, True, no_chains)
    up = tr.info(n, rp, ci, va, False, False, no_chains)
    return {"n": n, "nnz": int(rp[n]), "levels": low["levels"], "widest_level": low["widest_level"], "launches_per_factor": low["launches_per_solve"],
            "chains": low["chains"], "launches_per_apply": low["launches_per_solve"] + up["launches_per_solve"], "bad_row": -1,
            "bad_pivot": factor(n, rp, ci, va)[1]}


HOST_WAITS_SLACK = 13   # host_waits <= launches / 16 + 13 (g4s.h)


def dense(n, rp, ci, va):
    return tr.dense(n, rp, ci, va)


def split(n, rp, ci, f):
    """(L with its unit diagonal, U) as dense arrays"""
    a = tr.dense(n, rp, ci, f)
    return np.tril(a, -1) + np.eye(n), np.triu(a)


def pcg(n, rp, ci, va, b, f=None, tol=1e-10, maxiter=None):
    """host.pcg restated on dense numpy: (x, iterations, relative residual)"""
    a = tr.dense(n, rp, ci, va)
    M = (lambda r: r.copy()) if f is None else (lambda r: apply(n, rp, ci, f, r))
    x, r = np.zeros(n), np.array(b, np.float64)
    bnorm = np.linalg.norm(b)
    z = M(r)
    p, rz, it = z.copy(), r @ z, 0
    while np.linalg.norm(r) > tol * bnorm and it < (n if maxiter is None else maxiter):
        q = a @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        it += 1
        if np.linalg.norm(r) <= tol * bnorm:
            break
        z = M(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it, np.linalg.norm(r) / bnorm


# ------------------------------------------------------------------------------------------------------------------------------------ the cases
def _rng(seed):
    return np.random.default_rng(seed)


def canonical(rows):
    """rows sorted by column, the first of repeated columns kept"""
    out = []
    for r in rows:
        seen = {}
        for c, v in r:
            seen.setdefault(c, v)
        out.append(sorted(seen.items()))
    return out


def dominant(rows, margin=1.0):
    """the diagonal entry of every row set to margin + the sum of the row's other magnitudes: no pivot comes near zero"""
    return [[(c, margin + sum(abs(w) for d, w in r if d != i) if c == i else v) for c, v in r] for i, r in enumerate(rows)]


def tridiagonal(n, seed=21):
    rng = _rng(seed)
    return tr.csr(dominant([[(j, float(rng.uniform(-1, 1)) if j != i else 0.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]))


def laplace5(nx):
    """the five-point Laplacian of an nx × nx grid: 4 on the diagonal, −1 beside it; symmetric positive definite, 2·nx − 1 levels of widths 1 … nx … 1"""
    rows = []
    for y in range(nx):
        for x in range(nx):
            i = y * nx + x
            rows.append([(j, -1.0) for j, ok in ((i - nx, y > 0), (i - 1, x > 0)) if ok] + [(i, 4.0)]
                        + [(j, -1.0) for j, ok in ((i + 1, x < nx - 1), (i + nx, y < nx - 1)) if ok])
    return tr.csr(rows)


def full(n, seed=22):
    rng = _rng(seed)
    return tr.csr(dominant([[(j, float(rng.uniform(-1, 1))) for j in range(n)] for _ in range(n)]))


def blocks(widths, seed=23):
    """the lower triangle of trsv_ref.blocks — levels of the given widths — made canonical, and its transposed pattern above the diagonal with values
    of its own: the lower DAG keeps its levels, and a pivot row has entries to update with"""
    rng = _rng(seed)
    n, rp, ci, va = tr.blocks(widths)
    rows = canonical([[(int(ci[k]), float(va[k])) for k in range(rp[i], rp[i + 1])] for i in range(n)])
    for i in range(n):
        for c, _ in list(rows[i]):
            if c < i:
                rows[c].append((i, float(rng.uniform(-1, 1))))
    return tr.csr(dominant(canonical(rows)))


def arrow(n, seed=24):
    """the last row and the last column full, a band at +1 and +3 above the diagonal: two levels, the second the one long row n − 1 of n entries,
    whose every pivot row has up to three entries behind its diagonal"""
    rng = _rng(seed + n)
    rows = [sorted({i, min(i + 1, n - 1), min(i + 3, n - 1), n - 1}) for i in range(n - 1)] + [list(range(n))]
    return tr.csr(dominant([[(j, float(rng.uniform(-1, 1))) for j in r] for r in rows]))


def two_long_rows(base=WAVE_ROW + 8, seed=29):
    """`base` short rows with a band at +1 and +3 and the last two columns full, then two rows that store all of the first `base` columns and their
    own diagonal: both are above WAVE_ROW, neither reads the other, so they share a level — and a tile"""
    rng = _rng(seed)
    rows = [sorted({i, min(i + 1, base - 1), min(i + 3, base - 1), base, base + 1}) for i in range(base)] + [list(range(base)) + [base + h] for h in range(2)]
    return tr.csr(dominant([[(j, float(rng.uniform(-1, 1))) for j in r] for r in rows]))


def strided_tiles(base=16, rows=300, seed=30):
    """the pattern of trsv_ref's strided_tiles made canonical: `base` short rows with a band at +1 and +3 and one column each among the later rows'
    diagonals, then `rows` rows that store all of the first `base` columns and their own diagonal. One level of `rows` wave rows with `base` pivots
    each: its launch gives a workgroup eight of them, two a wave, and the last workgroup four"""
    rng = _rng(seed)
    pat = [sorted({i, min(i + 1, base - 1), min(i + 3, base - 1), base + (rows // base) * i}) for i in range(base)] + [list(range(base)) + [base + h] for h in range(rows)]
    return tr.csr(dominant([[(j, float(rng.uniform(-1, 1))) for j in r] for r in pat]))


def row0_full(n=200, seed=25):
    """row 0 is full; every later row stores (i, 0), its diagonal and up to two more columns (every tenth row a dozen): the pivot step on row 0 walks
    n − 1 entries, mostly onto columns the row does not store"""
    rng = _rng(seed)
    rows = [[(j, float(rng.uniform(-1, 1))) for j in range(n)]]
    for i in range(1, n):
        more = rng.integers(1, n, 12 if i % 10 == 0 else int(rng.integers(0, 3)))
        rows.append([(int(j), float(rng.uniform(-1, 1))) for j in sorted({0, i, *map(int, more)})])
    return tr.csr(dominant(rows))


def messy(n=60, seed=26):
    """a random unsymmetric canonical pattern: up to eight columns a row beside the diagonal, so most updates of a pivot row are dropped"""
    rng = _rng(seed)
    return tr.csr(dominant([[(int(j), float(rng.uniform(-1, 1))) for j in sorted({i, *map(int, rng.integers(0, n, int(rng.integers(0, 9))))})] for i in range(n)]))


def zero_pivot():
    """u_22 = 1 − 1·1 is an exact zero in row 2; rows 3 and 4 divide by it (±inf) and row 4 then divides inf by inf (NaN); rows 5 and 6 do not
    meet it and stay finite, row 5 with a −0.0"""
    return tr.csr([[(0, 2.0), (1, 1.0)],
                   [(0, 2.0), (1, 2.0), (2, 1.0), (3, 1.0), (5, 0.0)],
                   [(1, 1.0), (2, 1.0), (3, 3.0), (4, 1.0)],
                   [(2, 1.0), (3, 1.0), (4, 2.0)],
                   [(2, -1.0), (3, 1.0), (4, 1.0)],
                   [(1, 1.0), (3, 1.0), (5, 1.0)],
                   [(0, 1.0), (6, 4.0)]])


def with_specials(seed=27):
    """`messy` with a NaN, an inf and a −0.0 stored in A"""
    n, rp, ci, va = messy(40, seed)
    va = va.copy()
    rowid = np.repeat(np.arange(n), np.diff(rp))
    off = np.flatnonzero(ci != rowid)
    va[off[3]], va[off[len(off) // 2]], va[off[-2]] = np.nan, np.inf, -0.0
    return n, rp, ci, va


def exact_full(n=12, seed=28):
    """A = L0 U0 with a unit lower L0 of small integers and an upper U0 of small integers with a power-of-two diagonal, on the full pattern: every
    intermediate of the factorisation is an integer or a dyadic rational far inside 53 bits, and the factors are L0 and U0 themselves"""
    rng = _rng(seed)
    L0 = np.tril(rng.integers(-2, 3, (n, n)), -1).astype(np.float64) + np.eye(n)
    U0 = np.triu(rng.integers(-2, 3, (n, n)), 1).astype(np.float64) + np.diag(2.0 ** rng.integers(0, 3, n))
    a = L0 @ U0
    return tr.csr([[(j, float(a[i, j])) for j in range(n)] for i in range(n)]), L0, U0


CASES = {
    "n0": lambda: tr.csr([]),
    "n1": lambda: tr.csr([[(0, 2.5)]]),
    "diagonal_300": lambda: tr.csr([[(i, 1.0 + i)] for i in range(300)]),
    "tridiagonal_cap_minus_1": lambda: tridiagonal(CHAIN_LEVELS - 1),
    "tridiagonal_cap": lambda: tridiagonal(CHAIN_LEVELS),
    "tridiagonal_cap_plus_1": lambda: tridiagonal(CHAIN_LEVELS + 1),
    "grid40": lambda: laplace5(40),
    "dense_70": lambda: full(70),
    "blocks": lambda: blocks([CHAIN_WIDTH - 1, CHAIN_WIDTH, CHAIN_WIDTH + 1, CHAIN_WIDTH, CHAIN_WIDTH - 1, CHAIN_WIDTH + 1, 5]),
    "arrow_lane_minus_1": lambda: arrow(LANE_ROW - 1),
    "arrow_lane": lambda: arrow(LANE_ROW),
    "arrow_lane_plus_1": lambda: arrow(LANE_ROW + 1),
    "arrow_wave_minus_1": lambda: arrow(WAVE_ROW - 1),
    "arrow_wave": lambda: arrow(WAVE_ROW),
    "arrow_wave_plus_1": lambda: arrow(WAVE_ROW + 1),
    "two_long_rows": lambda: two_long_rows(),
    "strided_tiles": lambda: strided_tiles(),
    "row0_full": lambda: row0_full(),
    "messy": lambda: messy(),
    "zero_pivot": lambda: zero_pivot(),
    "specials": lambda: with_specials(),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(matrix, factors, info, r, z) of a named case: built, factorised and applied once, shared and read-only"""
    mat = CASES[name]()
    n = mat[0]
    f, _ = factor(*mat)
    r = _rng(200 + len(name)).uniform(-1.0, 1.0, n)
    out = (mat, f, info(*mat), r, apply(*mat[:3], f, r))
    for a in mat[1:] + (f, r, out[4]):
        a.setflags(write=False)
    return out
