"""Inputs for the row-streaming SpMV path (g4s_amd/csrc/spmv.hip, plan format in spmv_stream.hpp; spmv_path 0) that sit ON its thresholds — the
lanes-per-row reduction, the heavy-row side list, the long-row chunk loops, the XCD remap of the block index, both plan builders — plus a numpy
restatement of the plan rules: which blocks each builder must produce, how the kernel reduces each block and which lane(s) sum each row.
numpy only: no GPU, no torch.

tests/test_stream_cases_cpu.py proves that every case reaches the edge its name claims and that the union covers every edge;
tests/test_spmv_stream_gpu.py runs them (SpMV, semiring SpMV and SpMM, on the host-built and the device-built plan)."""
import functools
from typing import Callable, NamedTuple

import numpy as np

# ---- the plan's constants: exported through g4s_csr_get_info (tile_nnz, tile_rows, long_chunk_nnz); the GPU test checks these defaults against it
TILE_NNZ = 2048              # spmv_stream.hpp: `constexpr int TILE_NNZ = 2048;` — entries per stream block
TILE_ROWS = 1024             # spmv_stream.hpp: `#define G4S_TILE_ROWS 1024` — rows per stream block
LONG_CHUNK = 2048            # spmv_stream.hpp: `constexpr int LONG_CHUNK = 2048;` — entries per chunk of a row longer than TILE_NNZ
# ---- not exported, each beside the source line it mirrors
WG = 256                     # spmv.hip: `constexpr int WG = 256;`
SHORT_ROWS_FACTOR = 16       # spmv_csr_adaptive_kernel: `if (nrows * 2 > WG || nnzb <= 16 * nrows)` → one lane per row
MAX_TPR = 64                 # the else branch: `int tpr = 64; while (tpr * nrows > WG) tpr >>= 1;`
LANE_ROW_MAX = 64            # spmv.hip: `constexpr int kLaneRowMax = 64;` — `if (b - a > kLaneRowMax)` → the heavy list, one wavefront per row
HEAVY_CAP = TILE_NNZ // LANE_ROW_MAX   # `__shared__ int heavy[TILE_NNZ / kLaneRowMax]` = 32 slots (33 rows of 65 entries do not fit a block)
PLAN_RUN = 4096              # spmv.hip: `constexpr int kPlanRun = 4096;` — plan_walk_kernel: `const int end = min(rows, r + kPlanRun);`
XCDS = 8                     # common.hpp: `constexpr int kXcds = 8;` — finish_plan: stream_per_xcd, chunks_pad; the kernel's `lb = (bid % 8) * stream_per_xcd + bid / 8`
CHUNK_UNROLL = 4             # the chunk branch: `for (; k + 3 * WG < c.k1; k += 4 * WG)`, then `for (; k < c.k1; k += WG)`


class Plan(NamedTuple):
    blocks: list             # (row0, nrows, nnz) in row order
    long_rows: list          # rows of more than TILE_NNZ entries, ascending
    chunks: list             # (row, k0, k1) in slot order


class CSRArrays(NamedTuple):
    rowptr: np.ndarray       # int32, rows + 1
    colids: np.ndarray       # int32, ascending and distinct inside a row
    values: np.ndarray       # float64, U(−1, 1)
    rows: int
    cols: int
    x: np.ndarray            # float64, U(−1, 1), cols long
    shared: int              # the shared columns are [rows, rows + shared)


# ------------------------------------------------------------------------------------------------ the plan, restated
def _build(rowptr, run, tile_nnz, tile_rows, long_chunk):
    """stream_build's greedy rule applied inside runs of `run` rows: a block starts at the first row not yet placed and takes rows while the entry
    count stays <= tile_nnz, the row count <= tile_rows and the run has rows left; a row of more than tile_nnz entries is a long row on its own."""
    rp = np.asarray(rowptr, np.int64)
    rows = len(rp) - 1
    blocks, long_rows, chunks = [], [], []
    r = 0
    while r < rows:
        k0 = int(rp[r])
        if rp[r + 1] - k0 > tile_nnz:
            long_rows.append(r)
            chunks += [(r, k, min(k + long_chunk, int(rp[r + 1]))) for k in range(k0, int(rp[r + 1]), long_chunk)]
            r += 1
            continue
        end = min(rows, (r // run + 1) * run, r + tile_rows)
        e = int(np.searchsorted(rp, k0 + tile_nnz, side="right")) - 1     # the last row boundary with rowptr[e] − k0 <= tile_nnz
        e = max(r + 1, min(e, end))
        blocks.append((r, e - r, int(rp[e]) - k0))
        r = e
    return Plan(blocks, long_rows, chunks)


def host_blocks(rowptr, tile_nnz=TILE_NNZ, tile_rows=TILE_ROWS, long_chunk=LONG_CHUNK):
    """The plan of stream_build (host): one greedy pass over all rows."""
    return _build(rowptr, len(rowptr), tile_nnz, tile_rows, long_chunk)


def device_blocks(rowptr, tile_nnz=TILE_NNZ, tile_rows=TILE_ROWS, long_chunk=LONG_CHUNK):
    """The plan of stream_build_device / plan_walk_kernel: the host rule inside each run of PLAN_RUN rows, a forced cut at every run end. Long rows
    are the host's."""
    return _build(rowptr, PLAN_RUN, tile_nnz, tile_rows, long_chunk)


def tpr_of(nrows):
    """Lanes per row of a block that takes the shuffle branch: the largest power of two <= 64 with tpr·nrows <= WG."""
    tpr = MAX_TPR
    while tpr * nrows > WG:
        tpr >>= 1
    return tpr


def reduction_of(block, rowptr):
    """How spmv_csr_adaptive_kernel reduces a stream block: ("lane", []), ("lane+heavy", heavy rows) or (("group", tpr), [])."""
    row0, nrows, nnz = block
    if nrows * 2 > WG or nnz <= SHORT_ROWS_FACTOR * nrows:
        lens = np.diff(np.asarray(rowptr[row0:row0 + nrows + 1], np.int64))
        heavy = [row0 + int(i) for i in np.flatnonzero(lens > LANE_ROW_MAX)]
        assert len(heavy) <= HEAVY_CAP, "more heavy rows than a block of TILE_NNZ entries can hold"
        return ("lane+heavy", heavy) if heavy else ("lane", [])
    assert tpr_of(nrows) >= 2
    return ("group", tpr_of(nrows)), []


def row_kinds(rowptr, plan):
    """Per row, who sums it: "lane" (one lane, left to right: the oracle's order, bit-identical), "group" (tpr lanes + shuffles), "wave" (a heavy
    row: one wavefront) or "chunked" (a long row: one workgroup per chunk + the fix-up)."""
    kinds = np.empty(len(rowptr) - 1, dtype=object)
    kinds[np.asarray(plan.long_rows, np.int64)] = "chunked"
    for b in plan.blocks:
        kind, heavy = reduction_of(b, rowptr)
        kinds[b[0]:b[0] + b[1]] = "lane" if isinstance(kind, str) else "group"
        kinds[np.asarray(heavy, np.int64)] = "wave"
    assert all(k is not None for k in kinds)
    return kinds


def row_block(plan, rows):
    """Per row, the index of its stream block (−1: a long row)."""
    out = np.full(rows, -1, np.int64)
    for i, (r0, n, _) in enumerate(plan.blocks):
        out[r0:r0 + n] = i
    return out


def chunk_loops(n):
    """What a chunk of n entries asks of the chunk branch's two loops: lane t starts at k = t, runs the 4×-unrolled loop while k + 3·WG < n, then the
    WG-stride tail while k < n. Returns (unrolled trips, tail trips) of lane 0, and the set of such pairs over all 256 lanes."""
    def trips(t):
        k, u, s = t, 0, 0
        while k + (CHUNK_UNROLL - 1) * WG < n:
            k, u = k + CHUNK_UNROLL * WG, u + 1
        while k < n:
            k, s = k + WG, s + 1
        return u, s
    return trips(0), {trips(t) for t in range(WG)}


def _left_to_right(p):
    """0.0 + p[0] + p[1] + …, one fp64 addition at a time."""
    return np.add.accumulate(np.concatenate([[0.0], p]))[-1]


def _strided(p, lanes):
    """The private sums of `lanes` lanes: lane l adds p[l], p[l + lanes], … to 0.0 in that order. (The pad is +0.0, added last: it changes no bit.)"""
    q = np.concatenate([np.zeros(lanes), p, np.zeros(-len(p) % lanes)]).reshape(-1, lanes)
    return np.add.accumulate(q, axis=0)[-1]


def _shuffle_tree(v):
    """Lane 0 of an aligned group after `for (off = n/2; off > 0; off >>= 1) s += __shfl_down(s, off)`: at every step lane l adds lane l + off."""
    v, off = v.copy(), len(v) // 2
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return v[0]


def emulate_spmv(m, plan, x=None):
    """y = A·x in the additions the kernels of spmv.hip make, in their order (no atomics, -ffp-contract=off: the order is the source's): a "lane"
    row left to right; a "group" row as tpr strided private sums and the shuffle tree; a "wave" row the same with 64 lanes; a chunk as 256 strided
    private sums, one tree per wavefront, (w0 + w1) + (w2 + w3), and spmv_long_fixup_kernel adds a row's chunk sums to 0.0 in chunk order."""
    rp = m.rowptr.astype(np.int64)
    prod = m.values * (m.x if x is None else x)[m.colids]
    y = np.zeros(m.rows)
    for b in plan.blocks:
        kind, heavy = reduction_of(b, m.rowptr)
        for r in range(b[0], b[0] + b[1]):
            p = prod[rp[r]:rp[r + 1]]
            if isinstance(kind, tuple):
                y[r] = _shuffle_tree(_strided(p, kind[1]))
            elif r in heavy:
                y[r] = _shuffle_tree(_strided(p, 64))
            else:
                y[r] = _left_to_right(p)
    partial = {}
    for r, k0, k1 in plan.chunks:
        lanes = _strided(prod[k0:k1], WG)
        w = [_shuffle_tree(lanes[i:i + 64]) for i in range(0, WG, 64)]
        partial.setdefault(r, []).append((w[0] + w[1]) + (w[2] + w[3]))
    for r, parts in partial.items():
        y[r] = _left_to_right(np.array(parts))
    return y


def launch_geometry(plan):
    """(chunks_pad, stream_per_xcd, grid) of finish_plan / stream_spmv."""
    pad = -(-len(plan.chunks) // XCDS) * XCDS
    per = -(-len(plan.blocks) // XCDS)
    return pad, per, pad + per * XCDS


def remap(bid, plan):
    """The block a stream workgroup takes (None: it returns), `lb = (bid % kXcds) * stream_per_xcd + bid / kXcds`."""
    _, per, _ = launch_geometry(plan)
    lb = (bid % XCDS) * per + bid // XCDS
    return lb if lb < len(plan.blocks) else None


# ------------------------------------------------------------------------------------------------ matrices from row lengths
def _distinct(rng, n, k):
    """k distinct ids of [0, n), ascending."""
    if k == 0:
        return np.zeros(0, np.int64)
    if 4 * k >= n:
        return np.sort(rng.choice(n, k, replace=False))
    u = np.unique(rng.integers(0, n, size=k + k // 2 + 8))
    while len(u) < k:
        u = np.unique(np.concatenate([u, rng.integers(0, n, size=k)]))
    return u[np.sort(rng.permutation(len(u))[:k])]


def private_cols(m, r):
    """The columns that row r alone references: its first entry (column r) and, from two entries on, its last (column rows + shared + r)."""
    n = int(m.rowptr[r + 1] - m.rowptr[r])
    return [r][:n] + ([m.rows + m.shared + r] if n >= 2 else [])


def matrix_from_lens(lens, shared, seed):
    """Row r holds lens[r] entries: column r first, column rows + shared + r last (both its own), seeded distinct columns of the shared range
    [rows, rows + shared) between them. A NaN in x on a private column therefore reaches exactly one row, from the row's first or last product."""
    lens = np.asarray(lens, np.int64)
    rows = len(lens)
    assert lens.min(initial=0) >= 0 and lens.max(initial=0) - 2 <= shared
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    colids = np.empty(rowptr[-1], np.int64)
    for r in np.flatnonzero(lens):
        n = int(lens[r])
        colids[rowptr[r]] = r
        if n >= 2:
            colids[rowptr[r] + 1:rowptr[r + 1] - 1] = rows + _distinct(rng, shared, n - 2)
            colids[rowptr[r + 1] - 1] = rows + shared + r
    cols = 2 * rows + shared
    return CSRArrays(rowptr.astype(np.int32), colids.astype(np.int32), rng.uniform(-1, 1, colids.size), rows, cols, rng.uniform(-1, 1, cols), shared)


# ------------------------------------------------------------------------------------------------ row-length vectors
def _one_block(nrows, total, cap=LANE_ROW_MAX):
    """nrows row lengths that sum to `total`: row 1 empty and row 2 of one entry (from four rows on), the others level, none above `cap`."""
    if nrows < 4:
        lens = np.full(nrows, total // nrows)
        lens[0] += total - lens.sum()
        return lens
    lens = np.zeros(nrows, np.int64)
    lens[2] = 1
    free = np.array([r for r in range(nrows) if r not in (1, 2)])
    lens[free] = (total - 1) // len(free)
    lens[free[:(total - 1) % len(free)]] += 1
    assert lens.sum() == total and (cap is None or lens.max() <= cap)
    return lens


def _tpr_lens(nrows):
    """One block that takes the shuffle branch: rows of 17 entries where 17·nrows fits, else rows of 16 and one longer row that fills the block
    to TILE_NNZ; row 1 is empty and row 2 has one entry (nrows >= 4), which the first row makes up for."""
    if nrows < 4:
        return np.full(nrows, 17)
    if 17 * nrows <= TILE_NNZ:
        lens = np.full(nrows, 17)
        lens[0] += 17 + 16
    else:
        lens = np.full(nrows, 16)
        lens[0] = TILE_NNZ - 16 * (nrows - 3) - 1
    lens[1], lens[2] = 0, 1
    return lens


def _tpr_full_lens(nrows):
    """The same row counts with the block filled to TILE_NNZ by uneven rows (every lane of a group strides more than once)."""
    if nrows < 4:
        return _one_block(nrows, TILE_NNZ)
    rng = np.random.default_rng(1000 + nrows)
    lens = rng.multinomial(TILE_NNZ - 1, np.ones(nrows - 2) / (nrows - 2))
    return np.concatenate([lens[:1], [0, 1], lens[1:]])


def _switch_lens(nrows, over):
    lens = np.full(nrows, 16)
    lens[0] += 16 + 15                                                # 47 <= LANE_ROW_MAX: no heavy row on the one-lane side
    lens[1], lens[2] = 0, 1
    lens[3] += int(over)
    return lens


def _heavy_lens(n_heavy):
    """n_heavy rows of 65 entries, spread out, in one block of >= 129 rows filled to TILE_NNZ."""
    if n_heavy == 31:
        lens = np.array([65] * 31 + [1] * 33 + [0] * 65)
        return lens[np.random.default_rng(31).permutation(len(lens))]
    nrows = 160
    lens = _one_block(nrows - n_heavy, TILE_NNZ - 65 * n_heavy)
    at = np.linspace(5, nrows - n_heavy - 1, n_heavy).astype(int)     # before these short rows
    return np.insert(lens, at, 65)


def _heavy_64_65_lens():
    lens = _one_block(140, TILE_NNZ - 64 - 65, cap=63)                # every other row is clearly short
    return np.insert(lens, [70, 70], [64, 65])


def _long_among_short(*long_lens):
    lens = [3, 0]
    for n in long_lens:
        lens += [n, 5, 1]
    return np.array(lens)


def _nstream_lens(n):
    """Exactly n stream blocks under the host builder, no row empty: TILE_ROWS rows of one or two entries (the row cap ends the block) alternate
    with single rows of TILE_NNZ entries (a block each)."""
    short = np.tile([1, 2], TILE_ROWS // 2)
    parts = [short if i % 2 == 0 else np.array([TILE_NNZ]) for i in range(n)]
    return np.concatenate(parts)


def _run_lens(rows, fill=1, **at):
    lens = np.full(rows, fill)
    for r, n in at.items():
        lens[int(r[1:])] = n
    return lens


class Case(NamedTuple):
    name: str
    lens: Callable[[], np.ndarray]
    shared: int              # width of the shared column range
    claims: dict             # what tests/test_stream_cases_cpu.py proves about it


TPR_NROWS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127)
HEAVY_COUNTS = (1, 4, 5, 31)
CHUNK_TAILS = (1, 255, 256, 257, 769, 1023, 1024, 1025, 2048)
NSTREAM = (1, 7, 8, 9, 15, 16, 17)
SWITCH_NROWS = (8, 100)


def _cases():
    out = []
    for n in TPR_NROWS:
        out.append(Case(f"tpr_{n}", functools.partial(_tpr_lens, n), 5000, {"one_block": ("group", tpr_of(n)), "nrows": n}))
        out.append(Case(f"tpr_{n}_full", functools.partial(_tpr_full_lens, n), 5000, {"one_block": ("group", tpr_of(n)), "nrows": n, "nnz": TILE_NNZ}))
    for n in SWITCH_NROWS:
        out.append(Case(f"switch_16n_{n}_at", functools.partial(_switch_lens, n, False), 5000, {"one_block": "lane", "nrows": n, "nnz": 16 * n}))
        out.append(Case(f"switch_16n_{n}_over", functools.partial(_switch_lens, n, True), 5000, {"one_block": ("group", tpr_of(n)), "nrows": n, "nnz": 16 * n + 1}))
    out.append(Case("many_rows_129", lambda: _one_block(129, TILE_NNZ), 5000, {"one_block": "lane", "nrows": 129, "nnz": TILE_NNZ}))
    out.append(Case("rows_128_full", lambda: np.full(128, 16), 5000, {"one_block": "lane", "nrows": 128, "nnz": TILE_NNZ}))
    for n in HEAVY_COUNTS:
        out.append(Case(f"heavy_{n}", functools.partial(_heavy_lens, n), 5000, {"one_block": "lane+heavy", "heavy": n, "nnz": TILE_NNZ, "min_rows": 129}))
    out.append(Case("heavy_64_65", _heavy_64_65_lens, 5000, {"one_block": "lane+heavy", "heavy": 1, "nnz": TILE_NNZ, "min_rows": 129}))
    out.append(Case("heavy_few_rows", lambda: np.array([1] * 45 + [0] * 5 + [1500] + [0] * 4 + [1] * 45), 5000,
                    {"one_block": "lane+heavy", "heavy": 1, "nrows": 100, "nnz": 1590}))
    for L in CHUNK_TAILS:
        out.append(Case(f"chunk_tail_{L}", functools.partial(_long_among_short, LONG_CHUNK + L), 5000, {"chunks": 2, "tail": L}))
    # a row of more than TILE_NNZ = LONG_CHUNK entries has at least two chunks: n_chunks == 1 cannot be reached, 2 is the fewest
    out.append(Case("chunks_2", functools.partial(_long_among_short, 2049), 5000, {"chunks": 2}))
    out.append(Case("chunks_8", functools.partial(_long_among_short, 2049, 3 * LONG_CHUNK + 5, 2050), 8000, {"chunks": 8}))
    out.append(Case("chunks_9", functools.partial(_long_among_short, 8 * LONG_CHUNK + 1), 20000, {"chunks": 9}))
    out.append(Case("only_long_rows", lambda: np.array([2049, 4097, 2500]), 5000, {"chunks": 7, "n_stream": 0}))
    for n in NSTREAM:
        out.append(Case(f"nstream_{n}", functools.partial(_nstream_lens, n), 5000, {"n_stream": n, "no_empty_row": True}))
    R = PLAN_RUN
    out.append(Case("run_4096_ones", lambda: _run_lens(R), 100, {"host": 4, "device": 4, "cap_at_run_end": True}))
    out.append(Case("run_4097_ones", lambda: _run_lens(R + 1), 100, {"host": 5, "device": 5}))
    out.append(Case("run_2048_end0", lambda: _run_lens(R + 40, r4095=TILE_NNZ), 5000, {"len_at": (R - 1, TILE_NNZ)}))
    out.append(Case("run_2049_end0", lambda: _run_lens(R + 40, r4095=TILE_NNZ + 1), 5000, {"len_at": (R - 1, TILE_NNZ + 1)}))
    out.append(Case("run_2048_start1", lambda: _run_lens(R + 40, r4096=TILE_NNZ), 5000, {"len_at": (R, TILE_NNZ)}))
    out.append(Case("run_2049_start1", lambda: _run_lens(R + 40, r4096=TILE_NNZ + 1), 5000, {"len_at": (R, TILE_NNZ + 1)}))
    # run 1 holds no entry. Host: 6 blocks of 682 rows, then rows 4092.. with the empty rows that follow up to the row cap, 3 blocks of empty rows and
    # the rest (11); device: the cut at row 4096 ends the 4-row block, run 1 is 4 blocks of 1024 empty rows, run 2 one block of 3 rows (12)
    out.append(Case("run_empty_run", lambda: np.concatenate([np.full(R, 3), np.zeros(R, np.int64), [2, 0, 1]]), 100,
                    {"host": 11, "device": 12, "empty_run": 1}))
    # rows of 3 entries: 682 to a block (2046 entries). 8192 rows are 12 blocks and one of 8 rows on the host; each run of 4096 is 6 blocks and
    # one of 4 rows on the device: one block more, left by the forced cut at row 4096
    out.append(Case("run_forced_cut", lambda: _run_lens(2 * R, fill=3), 100, {"host": 13, "device": 14}))
    out.append(Case("run_equal_counts", lambda: _run_lens(2 * R, fill=2), 100, {"host": 8, "device": 8, "cap_at_run_end": True}))
    out.append(Case("empty_everything", lambda: np.zeros(2050, np.int64), 10, {"host": 3, "device": 3, "nnz": 0}))
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]
_BY_NAME = {c.name: c for c in CASES}
assert len(_BY_NAME) == len(CASES)

# the subsets the GPU test runs beyond plain SpMV
SEMIRING_NAMES = [n for n in NAMES if n.startswith(("tpr_", "switch_16n", "heavy_", "chunk_tail_", "only_long_rows"))]
SPMM_NAMES = ["chunk_tail_1", "chunk_tail_2048", "chunks_9", "only_long_rows", "tpr_5", "tpr_127", "heavy_31", "nstream_9"]


def case(name):
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def build(name):
    """The case's matrix and x (cached: treat as read-only)."""
    c = _BY_NAME[name]
    m = matrix_from_lens(c.lens(), c.shared, seed=NAMES.index(name) + 1)
    for a in (m.rowptr, m.colids, m.values, m.x):
        a.setflags(write=False)
    return m
