"""A plain numpy / Python restatement of the contract of g4s_sptrsv_* (include/g4s.h): which entries belong to the triangle, the levels, the (level, id)
schedule, the chaining rule that gives launches_per_solve and chains, and the solve in the documented arithmetic shape — the lane sum, the wave shape
of a long row and the workgroup shape of a hub row — so that the device's x can be compared bit for bit. test_trsv_cpu.py pins it to scipy and to a
longest-path computation; test_trsv_gpu.py compares the device with it. The cases are built once and shared; nobody writes to them."""
import functools

import numpy as np

WAVE_ROW, CHAIN_WIDTH, CHAIN_LEVELS, HUB_ROW = 32, 256, 1024, 4096


def csr(rows, n=None):
    """(n, rowptr, colids, values) from a list of rows, each a list of (col, value) in stored order"""
    n = len(rows) if n is None else n
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float64)
    return n, rp, ci, va


def triangle(n, rp, ci, va, lower=True, unit=False):
    """per row: (the off-diagonal triangle entries as (col, value, position) in stored order, the kept diagonal entries as (value, position))"""
    off, dia = [], []
    for i in range(n):
        o, d = [], []
        for k in range(int(rp[i]), int(rp[i + 1])):
            c = int(ci[k])
            if c == i:
                if not unit:
                    d.append((va[k], k))
            elif (c < i) == bool(lower):
                o.append((c, va[k], k))
        off.append(o)
        dia.append(d)
    return off, dia


def bad_row(n, rp, ci, va, lower=True, unit=False):
    """the smallest row that stores no diagonal entry, −1 when there is none (or the diagonal is unit)"""
    if unit:
        return -1
    _, dia = triangle(n, rp, ci, va, lower, unit)
    return next((i for i in range(n) if not dia[i]), -1)


def levels(n, rp, ci, va, lower=True, unit=False):
    """level[i] = 0 without off-diagonal triangle entries, else 1 + the largest level among their columns"""
    off, _ = triangle(n, rp, ci, va, lower, unit)
    lev = np.zeros(n, np.int32)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        if off[i]:
            lev[i] = 1 + max(int(lev[c]) for c, _, _ in off[i])
    return lev


def schedule(lev):
    """(rows in (level, id) order, the offsets of the levels in that order)"""
    order = np.argsort(lev, kind="stable").astype(np.int32)
    nlev = int(lev.max()) + 1 if lev.size else 0
    loff = np.zeros(nlev + 1, np.int64)
    loff[1:] = np.cumsum(np.bincount(lev, minlength=nlev)) if lev.size else 0
    return order, loff


def launch_plan(lev, no_chains=False):
    """The launches of one solve, as (first level, one past the last level, is a chain). A level of at most CHAIN_WIDTH rows is narrow; a maximal run of
    consecutive narrow levels is cut from its first level on into pieces of at most CHAIN_LEVELS levels, each one chain; every other level is one launch."""
    _, loff = schedule(lev)
    width = np.diff(loff)
    out, l = [], 0
    while l < width.size:
        e = l + 1
        narrow = not no_chains and width[l] <= CHAIN_WIDTH
        if narrow:
            while e < width.size and e - l < CHAIN_LEVELS and width[e] <= CHAIN_WIDTH:
                e += 1
        out.append((l, e, narrow))
        l = e
    return out


def info(n, rp, ci, va, lower=True, unit=False, no_chains=False):
    """the fields of g4s_trsv_info that are a function of the matrix and the flags"""
    off, dia = triangle(n, rp, ci, va, lower, unit)
    lev = levels(n, rp, ci, va, lower, unit)
    plan = launch_plan(lev, no_chains)
    return {"n": n, "nnz_triangle": sum(len(o) for o in off) + sum(len(d) for d in dia), "levels": int(lev.max()) + 1 if n else 0,
            "widest_level": int(np.bincount(lev).max()) if n else 0, "launches_per_solve": len(plan), "chains": sum(1 for _, _, c in plan if c),
            "bad_row": -1}


def _ladder(a):
    """wave_sum of wave_reduce.hpp: 64 values, offsets 32, 16, … 1; lane 0's result"""
    a = list(a)
    o = 32
    while o:
        for l in range(o):
            a[l] = a[l] + a[l + o]
        o >>= 1
    return a[0]


def _strided(p, width):
    part = [np.float64(0.0)] * width
    for k, v in enumerate(p):
        part[k % width] = part[k % width] + v
    return part


def row_sum(p):
    """s_i of the products p (np.float64, in stored order) in the shape the header documents for their number"""
    m = len(p)
    if m <= WAVE_ROW:
        s = np.float64(0.0)
        for v in p:
            s = s + v
        return s
    if m <= HUB_ROW:
        return _ladder(_strided(p, 64))
    part = _strided(p, 256)
    w = [_ladder(part[64 * j:64 * j + 64]) for j in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def solve(n, rp, ci, va, b, lower=True, unit=False):
    """x with T x = b in the documented arithmetic: x[i] = (b[i] − s_i) / d_i, d_i the stored diagonal entries summed from the left; a NaN in its
    canonical form"""
    off, dia = triangle(n, rp, ci, va, lower, unit)
    x = np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        for i in (range(n) if lower else range(n - 1, -1, -1)):
            s = row_sum([np.float64(v) * x[c] for c, v, _ in off[i]])
            t = np.float64(b[i]) - s
            if not unit:
                d = np.float64(dia[i][0][0])
                for v, _ in dia[i][1:]:
                    d = d + np.float64(v)
                t = t / d
            x[i] = np.float64("nan") if np.isnan(t) else t                   # a NaN is stored as 0x7FF8000000000000 (g4s.h)
    return x


def dense(n, rp, ci, va):
    a = np.zeros((n, n), np.float64)
    for i in range(n):
        for k in range(int(rp[i]), int(rp[i + 1])):
            a[i, int(ci[k])] += va[k]
    return a


def gauss_seidel(n, rp, ci, va, b, x, sweeps=1, symmetric=False):
    """host.gauss_seidel on inputs whose every intermediate is exact in fp64 (the tests check that with fractions): r = b − A x as a dense product,
    the correction by `solve`, x + correction"""
    a = dense(n, rp, ci, va)
    x = np.array(x, np.float64)
    for _ in range(sweeps):
        for lower in ((True, False) if symmetric else (True,)):
            r = np.asarray(b, np.float64) - a @ x
            x = x + solve(n, rp, ci, va, r, lower)
    return x


# ------------------------------------------------------------------------------------------------------------------------------------ the cases
def _rng(seed):
    return np.random.default_rng(seed)


def _val(rng):
    return float(rng.uniform(-1.0, 1.0))


def _diag(rng):
    return float(rng.uniform(2.0, 3.0))


def bidiagonal(n, seed=1):
    rng = _rng(seed)
    return csr([([(i - 1, _val(rng))] if i else []) + [(i, _diag(rng))] for i in range(n)])


def dense_lower(n, seed=2):
    """every row stores its whole lower triangle: row lengths 0 … n − 1, every level one row; the diagonal keeps the solution of size one"""
    rng = _rng(seed)
    return csr([[(j, _val(rng)) for j in range(i)] + [(i, float(i + 1) * _diag(rng))] for i in range(n)])


def grid5(nx, seed=3):
    """the five-point stencil of an nx × nx grid, whole (both triangles): its lower triangle has 2·nx − 1 levels of widths 1 … nx … 1"""
    rng = _rng(seed)
    rows = []
    for y in range(nx):
        for x in range(nx):
            i = y * nx + x
            r = [(j, _val(rng)) for j, ok in ((i - nx, y > 0), (i - 1, x > 0)) if ok] + [(i, 4.0 + _diag(rng))]
            r += [(j, _val(rng)) for j, ok in ((i + 1, x < nx - 1), (i + nx, y < nx - 1)) if ok]
            rows.append(r)
    return csr(rows)


def blocks(widths, seed=4):
    """Levels of the given widths, ids interleaved: the first row of every level comes first (ids 0 … K − 1), the others follow in a random order. A row of
    level k stores the first row of level k − 1 and up to two more rows of lower levels and ids."""
    rng = _rng(seed)
    K = len(widths)
    lev = list(range(K)) + [int(v) for v in rng.permutation(np.repeat(np.arange(K), np.array(widths) - 1))]
    rows = []
    for i, k in enumerate(lev):
        r = []
        if k:
            r.append((k - 1, _val(rng)))
            for _ in range(int(rng.integers(0, 3))):
                j = int(rng.integers(0, i))
                if lev[j] < k:
                    r.append((j, _val(rng)))
        rows.append(r + [(i, _diag(rng))])
    return csr(rows)


def long_rows(counts, base, seed=5):
    """`base` rows that store their diagonal only, then one row per count with that many off-diagonal entries among them (scaled to keep x of size one)"""
    rng = _rng(seed)
    rows = [[(i, _diag(rng))] for i in range(base)]
    for m in counts:
        i = len(rows)
        cols = rng.permutation(base)[:m]
        rows.append([(int(c), _val(rng) / 8.0) for c in cols] + [(i, _diag(rng))])
    return csr(rows)


def messy(n, seed=6):
    """unsorted columns, repeated off-diagonal entries, repeated diagonal entries, entries of both triangles"""
    rng = _rng(seed)
    rows = []
    for i in range(n):
        r = [(int(rng.integers(0, n)), _val(rng)) for _ in range(int(rng.integers(0, 9)))]
        r += [(c, _val(rng)) for c, _ in r[:2]]                            # repeats
        r += [(i, _diag(rng)) for _ in range(1 + int(rng.integers(0, 3)))]   # one to three diagonal entries
        rows.append([r[j] for j in rng.permutation(len(r))])
    return csr(rows)


def full(n, seed=7):
    """a full unsymmetric matrix in a random column order"""
    rng = _rng(seed)
    return csr([[(int(j), float(n) * _diag(rng) if j == i else _val(rng)) for j in rng.permutation(n)] for i in range(n)])


def poison_other_triangle(mat, lower):
    n, rp, ci, va = mat
    rowid = np.repeat(np.arange(n), np.diff(rp))
    va = va.copy()
    va[(ci > rowid) if lower else (ci < rowid)] = np.nan
    return n, rp, ci, va


def mirror(mat):
    """The upper twin of a lower case (and back): row and column i become n − 1 − i, every row keeps its stored order and its values. The upper triangle of
    the result is the lower triangle of `mat` with the ids reversed: the same DAG, the same levels, the rows of a level in the opposite order."""
    n, rp, ci, va = mat
    rows = [[(n - 1 - int(ci[k]), float(va[k])) for k in range(int(rp[i]), int(rp[i + 1]))] for i in range(n - 1, -1, -1)]
    return csr(rows, n)


def unit_poisoned(n, seed=8):
    """a strictly-lower part; every second row also stores a NaN on the diagonal, the others store none"""
    rng = _rng(seed)
    rows = []
    for i in range(n):
        r = [(int(j), _val(rng) / 4.0) for j in rng.permutation(i)[:int(rng.integers(0, 6))]]
        if i % 2:
            r.insert(int(rng.integers(0, len(r) + 1)), (i, float("nan")))
        rows.append(r)
    return csr(rows)


def exact_case(n=48, seed=9, diag=2.0):
    """Whole matrix with small integer entries, a power-of-two diagonal and at most three levels in either triangle: every intermediate of a few solves and
    sweeps is a dyadic rational far inside 53 bits, so any summation order gives the same bits."""
    rng = _rng(seed)
    third = n // 3
    rows = []
    for i in range(n):
        band = i // third
        r = []
        for _ in range(int(rng.integers(0, 4))):
            j = int(rng.integers(0, n))
            if j // third != band:                                   # couples bands only: depth at most 3
                r.append((j, float(rng.integers(-1, 2))))
        r.insert(int(rng.integers(0, len(r) + 1)), (i, diag))
        rows.append(r)
    return csr(rows)


CASES = {
    "n0": lambda: csr([]),
    "n1": lambda: csr([[(0, 2.5)]]),
    "diagonal_300": lambda: csr([[(i, 1.0 + i)] for i in range(300)]),
    "bidiagonal_cap_minus_1": lambda: bidiagonal(CHAIN_LEVELS - 1),
    "bidiagonal_cap": lambda: bidiagonal(CHAIN_LEVELS),
    "bidiagonal_cap_plus_1": lambda: bidiagonal(CHAIN_LEVELS + 1),
    "dense_lower_70": lambda: dense_lower(70),
    "grid40": lambda: grid5(40),
    "blocks": lambda: blocks([CHAIN_WIDTH - 1, CHAIN_WIDTH, CHAIN_WIDTH + 1, CHAIN_WIDTH, CHAIN_WIDTH - 1, CHAIN_WIDTH + 1, 5]),
    "wave_row_edges": lambda: long_rows([WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, 63, 64, 65], 70),
    "hub_row": lambda: long_rows([HUB_ROW + 1, HUB_ROW], HUB_ROW + 3),
    # a level launch of several workgroups whose threads own a row only every stride-th: 300 rows of 17 entries are 64 rows a workgroup (stride 4), the
    # fifth workgroup 44; 260 rows of 257 entries are one row a wave (stride 64), 65 workgroups
    "strided_tiles": lambda: long_rows([16] * 300, 16),
    "wave_tiles": lambda: long_rows([256] * 260, 256),
    "messy": lambda: messy(60),
}


@functools.lru_cache(maxsize=None)
def case(name, lower=True, unit=False):
    """(matrix, level, info, b, x) of a named case: built and solved once, shared and read-only"""
    mat = CASES[name]()
    n = mat[0]
    b = _rng(100 + len(name)).uniform(-1.0, 1.0, n)
    out = (mat, levels(*mat, lower, unit), info(*mat, lower, unit), b, solve(*mat, b, lower, unit))
    for a in mat[1:] + (out[1], b, out[4]):
        a.setflags(write=False)
    return out
