"""Inputs for the two structured SpMV paths — the index-free diagonal path (g4s_amd/csrc/spmv_dia.hip, spmv_path 3) and the block-row path
(g4s_amd/csrc/spmv_bcsr.hip, spmv_path 4) — at every kernel instantiation and on both sides of every selection threshold, plus expected_path(),
a numpy restatement of the selection rules (dia_try_build, bcsr_try_build). numpy only: no GPU, no torch.

tests/test_structured_cases_cpu.py proves that every case has the property its name claims; tests/test_spmv_structured_gpu.py runs them."""
import functools
from typing import Callable, NamedTuple

import numpy as np

from tests.pb_cases import PATH_BLOCKED, PB_MIN_NNZ, PB_MIN_X_BYTES, should_use   # the blocked path's probe, restated beside its plan (tests/pb_cases.py)

# ---- selection thresholds, each beside the source line it mirrors
DIA_MIN_ROWS = 1024          # spmv_dia.hip, dia_try_build: `if (rows < 1024 || nnz < 4096) return G4S_OK;`
DIA_MIN_NNZ = 4096           # (the same line)
DIA_MAX_DIAGS = 32           # spmv_dia.hip: `constexpr int kMaxDiags = 32;` — `if ((int)offs.size() > kMaxDiags) return G4S_OK;`
DIA_MIN_FILL = 0.6           # dia_try_build: `(double)nnz < 0.6 * (double)nd * rows`
DIA_SAMPLE_ROWS = 2048       # dia_try_build: `const int S = 2048;` — the first, the middle and the last S rows give the candidate offsets
DIA_SAMPLE_MAX_LEN = 64      # dia_try_build: `if (k1 - k0 > 64ll * S) return G4S_OK;` — rows this long are not a stencil
BCSR_MIN_ROWS = 64           # spmv_bcsr.hip, bcsr_try_build: `if (rows < 64 || nnz <= 0) return G4S_OK;`
BCSR_ORDER = (3, 2)          # bcsr_try_build: `for (int b : {3, 2})` — the first block size that fits is taken; 4×4 blocks pass as 2×2
BCSR_MIN_BLOCKS = 2          # bcsr_try_build: `nnz < 2ll * b * rows` — two blocks per block-row on average
BCSR_TILE = 1024             # spmv_bcsr.hip: `#define G4S_BCSR_TILE 1024`; bcsr_check_kernel: `L / b <= tile_blocks`, tile_blocks = kTile / b²
BCSR_MAX_BROWS = 512         # spmv_bcsr.hip: `kMaxBrows = 512` — block-rows per work item
assert (PB_MIN_X_BYTES, PB_MIN_NNZ) == (8 << 20, 4 << 20)   # spmv_pb.hip, pb_should_use: `cols * 8 < (8ll << 20) || nnz < (4ll << 20)` → never the blocked path
DIA_WG = 256                 # spmv_dia.hip: `constexpr int WG = 256;`
XCDS = 8                     # common.hpp: kXcds — the grid of a diagonal launch is rounded up to a multiple of it

PATH_STREAM, PATH_DIAGONAL, PATH_BLOCKROW = 0, 3, 4


class CSRArrays(NamedTuple):
    rowptr: np.ndarray       # int32, rows + 1
    colids: np.ndarray       # int32
    values: np.ndarray       # float64
    rows: int
    cols: int


def tile_blocks(b):
    """The most blocks a block-row may hold: 256 / 113 / 64 for b = 2 / 3 / 4."""
    return BCSR_TILE // (b * b)


# ------------------------------------------------------------------------------------------------ generators
def diag_matrix(rows, cols, offsets, *, holes=0.0, empty_rows=(), seed, swap_in_row=None, duplicate_in_row=None):
    """One entry per (row, offset) inside the rows × cols matrix, rows sorted by column. `holes`: that fraction (an exact count, rounded) of the
    entries of interior rows — rows that hold every offset — is removed at random, entry by entry. `empty_rows` are emptied. Values U(−1, 1).
    swap_in_row=r exchanges the first two columns of row r (a descending pair), duplicate_in_row=r repeats the first column of row r."""
    offs = np.array(sorted(set(int(o) for o in offsets)), np.int64)
    assert len(offs) == len(list(offsets)), "offsets repeat"
    rng = np.random.default_rng(seed)
    col = np.arange(rows, dtype=np.int64)[:, None] + offs[None, :]
    present = (col >= 0) & (col < cols)
    interior = np.flatnonzero(present & present.all(axis=1)[:, None])
    n_holes = int(round(holes * interior.size))
    if n_holes:
        present.ravel()[rng.choice(interior, n_holes, replace=False)] = False
    present[list(empty_rows), :] = False
    rowptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.int32)
    colids = col[present].astype(np.int32)                           # row-major, offsets ascending: ascending columns in every row
    values = rng.uniform(-1, 1, colids.size)
    for r, what in ((swap_in_row, "swap"), (duplicate_in_row, "duplicate")):
        if r is None:
            continue
        k = int(rowptr[r])
        assert rowptr[r + 1] - k >= 2, "the row needs two entries"
        colids[k], colids[k + 1] = (colids[k + 1], colids[k]) if what == "swap" else (colids[k], colids[k])
    return CSRArrays(rowptr, colids, values, int(rows), int(cols))


def block_matrix(b, blocks_per_brow, n_bcols, *, seed, shift_run=None, descending=None, cols_extra=0, rows_extra=0):
    """Dense b×b blocks as bcsr_check_kernel expects them: block-row n holds blocks_per_brow[n] blocks (0 allowed) at random ascending block
    columns < n_bcols; each of its b rows lists the same columns, every block an aligned run of b. cols = b·n_bcols + cols_extra.
    shift_run=(brow, k) moves run k of that block-row one column to the right in all b rows (misaligned, nothing else changes; the block-row's
    block columns are then drawn from the even ones so that the run stays clear of its neighbour), descending=(brow,) exchanges its first two
    block columns, rows_extra appends empty rows (rows % b != 0)."""
    rng = np.random.default_rng(seed)
    cols = b * n_bcols + cols_extra
    lens, chunks = [], []
    for n, k in enumerate(blocks_per_brow):
        if shift_run is not None and shift_run[0] == n:
            bc = 2 * np.sort(rng.choice((n_bcols - 1 + cols_extra // b) // 2, k, replace=False))
        else:
            bc = np.sort(rng.choice(n_bcols, k, replace=False))
        if descending is not None and descending[0] == n:
            assert k >= 2
            bc[0], bc[1] = bc[1], bc[0]
        line = (bc[:, None] * b + np.arange(b)[None, :]).astype(np.int64)
        if shift_run is not None and shift_run[0] == n:
            line[shift_run[1]] += 1
        chunks.append(np.tile(line.ravel(), b))
        lens += [k * b] * b
    lens += [0] * rows_extra
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colids = (np.concatenate(chunks) if chunks else np.zeros(0)).astype(np.int32)
    assert colids.size == 0 or (colids.min() >= 0 and colids.max() < cols)
    return CSRArrays(rowptr, colids, rng.uniform(-1, 1, colids.size), len(lens), int(cols))


# ------------------------------------------------------------------------------------------------ the selection rules, restated
def row_of(rowptr):
    """The row of every entry."""
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr).astype(np.int64))


def dia_offsets(rows, cols, rowptr, colids):
    """The plan's offsets if dia_try_build keeps the diagonal form, else None."""
    rowptr = np.asarray(rowptr, np.int64)
    nnz = int(rowptr[-1])
    if rows < DIA_MIN_ROWS or nnz < DIA_MIN_NNZ:
        return None
    S = DIA_SAMPLE_ROWS
    offset = np.asarray(colids, np.int64) - row_of(rowptr)
    offs = np.zeros(0, np.int64)
    for ra in (0, max(0, rows // 2 - S // 2), max(0, rows - S)):      # candidate offsets: the first, the middle and the last S rows
        rb = min(rows, ra + S)
        if rowptr[rb] - rowptr[ra] > DIA_SAMPLE_MAX_LEN * S:
            return None
        offs = np.union1d(offs, offset[rowptr[ra]:rowptr[rb]])
        if offs.size > DIA_MAX_DIAGS:
            return None
    nd = int(offs.size)
    if nd == 0 or float(nnz) < DIA_MIN_FILL * float(nd) * rows:
        return None
    # the fill pass: every entry on a candidate diagonal, columns strictly ascending in every row (no repeat, no descending pair)
    idx = np.searchsorted(offs, offset)
    if np.any(idx >= nd) or np.any(offs[np.minimum(idx, nd - 1)] != offset):
        return None
    same_row = np.ones(nnz, bool)
    same_row[rowptr[:-1][rowptr[:-1] < nnz]] = False                 # the first entry of a row has no predecessor
    if np.any(same_row[1:] & (idx[1:] <= idx[:-1])):
        return None
    return offs


def bcsr_block(rows, cols, rowptr, colids):
    """The block size bcsr_try_build settles on, or 0."""
    rowptr, colids = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    nnz = int(rowptr[-1])
    if rows < BCSR_MIN_ROWS or nnz <= 0:
        return 0
    lens = np.diff(rowptr)
    row = row_of(rowptr)
    k = np.arange(nnz, dtype=np.int64) - rowptr[row]                 # position inside the row
    for b in BCSR_ORDER:
        if rows % b or cols % b or nnz % (b * b) or nnz < BCSR_MIN_BLOCKS * b * rows:
            continue
        L = lens.reshape(rows // b, b)
        if np.any(L != L[:, :1]) or np.any(L[:, 0] % b) or np.any(L[:, 0] // b > tile_blocks(b)):
            continue
        if np.any(colids != (colids // b) * b + k % b):              # aligned runs
            continue
        d = row % b                                                  # the b rows of a block-row hold the first row's columns
        if np.any(colids != colids[np.arange(nnz) - d * lens[row]]):
            continue
        head = (k % b == 0) & (k > 0)                                # block columns ascending
        if np.any(colids[head] <= colids[np.flatnonzero(head) - 1]):
            continue
        return b
    return 0


def expected_path(rows, cols, rowptr, colids, force_stream=False):   # force_stream: created with G4S_SPMV_STREAM
    """g4s_csr_info.spmv_path of a handle created from this matrix (csr.hip, g4s_csr_create): the diagonal form first, then the block-row form,
    else the row-streaming kernel. A matrix large enough for the blocked path's locality probe takes the blocked path where the probe says so
    (pb_cases.should_use), before the structured forms are tried."""
    nnz = int(rowptr[-1])
    if force_stream or nnz == 0:
        return PATH_STREAM
    if cols * 8 >= PB_MIN_X_BYTES and nnz >= PB_MIN_NNZ and should_use(rows, cols, nnz, colids)[0]:
        return PATH_BLOCKED
    if dia_offsets(rows, cols, rowptr, colids) is not None:
        return PATH_DIAGONAL
    return PATH_BLOCKROW if bcsr_block(rows, cols, rowptr, colids) else PATH_STREAM


def dia_workgroups(rows, two_rows):
    """(workgroups that hold rows, grid size) of the diagonal launch that covers most rows: the two-rows-per-lane kernel (y 16-byte aligned,
    at most 16 diagonals) or the one-row kernel. The grid is the workgroups rounded up to a multiple of the XCD count."""
    lanes = (rows & ~1) // 2 if two_rows else rows
    n = (lanes + DIA_WG - 1) // DIA_WG
    return n, (n + XCDS - 1) // XCDS * XCDS


# ------------------------------------------------------------------------------------------------ the cases
class Case(NamedTuple):
    name: str
    make: Callable[[], CSRArrays]
    path: int                # the path the case is built to take
    claims: dict             # what the name promises, checked by tests/test_structured_cases_cpu.py


def instantiation_offsets(nd):
    """nd offsets that are not contiguous: multiples of 3 around 0 and, from two on, one beyond +1000 and one beyond −1000 (boundary rows lose
    entries on both sides). nd == 1: the single offset 3 (used with cols = rows + 3, so that rows ≥ 4096 gives nnz ≥ 4096)."""
    if nd == 1:
        return (3,)
    m = nd - 2
    return tuple([-1003] + [3 * (j - m // 2) for j in range(m)] + [1001])


def _refresh_offsets(nd):
    return tuple(2 * (j - 3) for j in range(nd))                     # −6, −4, …: even offsets, no far ones (small matrices stay well filled)


INSTANTIATION_ND = (1, 8, 9, 16, 17, 32)
REFRESH_ND = (8, 9, 16, 17, 32)
_GEOMETRY_OFFSETS = (-70, -3, 0, 2, 65)
_FILL_OFFSETS = (-7, -2, 0, 3, 11)
_FILL_ROWS = 2000


def _fill_case(nnz_target):
    full = diag_matrix(_FILL_ROWS, _FILL_ROWS, _FILL_OFFSETS, seed=0)
    row_full = np.diff(full.rowptr) == len(_FILL_OFFSETS)
    interior = int(row_full.sum()) * len(_FILL_OFFSETS)
    return diag_matrix(_FILL_ROWS, _FILL_ROWS, _FILL_OFFSETS, holes=(len(full.colids) - nnz_target) / interior, seed=61)


def dia_cases():
    out = []
    add = lambda name, make, path, **claims: out.append(Case(name, make, path, claims))
    for nd in INSTANTIATION_ND:
        for rows in (4098, 4097):
            cols = rows + 3 if nd == 1 else rows
            add(f"inst_nd{nd}_rows{rows}", functools.partial(diag_matrix, rows, cols, instantiation_offsets(nd), seed=100 + nd), PATH_DIAGONAL,
                nd=nd, far_offsets=nd > 1)
    add("inst_nd33_rows4098", functools.partial(diag_matrix, 4098, 4098, instantiation_offsets(33), seed=133), PATH_STREAM, nd=33, far_offsets=True)
    # launch geometry: 2 (the fewest the 1024-row floor allows), 7, 8 and 9 workgroups of the two-row kernel: one XCD round of 8 not filled, filled, exceeded
    for rows, wgs in ((1024, 2), (2 * 256 * 6 + 2, 7), (2 * 256 * 7 + 2, 8), (2 * 256 * 8 + 2, 9)):
        add(f"geometry_{wgs}wg_rows{rows}", functools.partial(diag_matrix, rows, rows, _GEOMETRY_OFFSETS, seed=200 + wgs), PATH_DIAGONAL, nd=5, workgroups2=wgs)
    for rows in (64 * 20 + 1, 64 * 20 + 63):                           # ld = rows rounded up to 64
        add(f"geometry_ld_rows{rows}", functools.partial(diag_matrix, rows, rows, _GEOMETRY_OFFSETS, seed=rows), PATH_DIAGONAL, nd=5, ld_remainder=rows % 64)
    add("rect_tall_trailing_empty", functools.partial(diag_matrix, 3000, 2000, (0, 5, 130), seed=31), PATH_DIAGONAL, nd=3, trailing_empty=1000)
    add("rect_wide", functools.partial(diag_matrix, 2000, 3000, (-4, 0, 7, 900), seed=32), PATH_DIAGONAL, nd=4)
    add("interior_empty_run", functools.partial(diag_matrix, 3000, 3000, (-50, -9, -1, 0, 2, 10, 49), empty_rows=range(1500, 1540), seed=33), PATH_DIAGONAL,
        nd=7, empty_run=40)
    add("holes_fill_0.9", functools.partial(diag_matrix, 3000, 3000, (-50, -9, -1, 0, 2, 10, 49), holes=0.1, seed=34), PATH_DIAGONAL, nd=7, fill=(0.88, 0.92),
        masks_with_holes=True)
    # thresholds
    add("rows_1023", functools.partial(diag_matrix, 1023, 1023, (-3, -1, 0, 2, 5), seed=41), PATH_STREAM, nd=5)
    add("rows_1024", functools.partial(diag_matrix, 1024, 1024, (-3, -1, 0, 2, 5), seed=41), PATH_DIAGONAL, nd=5)
    add("nnz_4095", functools.partial(diag_matrix, 4096, 4096, (0,), empty_rows=(2000,), seed=42), PATH_STREAM, nd=1, nnz=4095)
    add("nnz_4096", functools.partial(diag_matrix, 4096, 4096, (0,), seed=42), PATH_DIAGONAL, nd=1, nnz=4096)
    thr = DIA_MIN_FILL * len(_FILL_OFFSETS) * _FILL_ROWS             # 6000 entries
    add("fill_just_above", functools.partial(_fill_case, int(thr) + 2), PATH_DIAGONAL, nd=5, nnz=int(thr) + 2, fill_side="above", masks_with_holes=True)
    add("fill_just_below", functools.partial(_fill_case, int(thr) - 2), PATH_STREAM, nd=5, nnz=int(thr) - 2, fill_side="below")
    # a descending pair / a repeated column in row 2500 of 8000: outside the sampled rows [0, 2048), [2976, 5024), [5952, 8000) — only the fill pass sees it
    add("swap_in_unsampled_row", functools.partial(diag_matrix, 8000, 8000, (-3, -1, 0, 2, 5), swap_in_row=2500, seed=43), PATH_STREAM, nd=5, odd_row=2500,
        unsorted=True)
    add("duplicate_in_unsampled_row", functools.partial(diag_matrix, 8000, 8000, (-3, -1, 0, 2, 5), duplicate_in_row=2500, seed=44), PATH_STREAM, nd=4 + 1,
        odd_row=2500, unsorted=True)
    # value refresh: holes, a run of interior empty rows, 40 trailing empty rows (rows beyond cols − min offset)
    for nd in REFRESH_ND:
        add(f"refresh_nd{nd}", functools.partial(diag_matrix, 2546, 2500, _refresh_offsets(nd), holes=0.15, empty_rows=range(1200, 1210), seed=300 + nd),
            PATH_DIAGONAL, nd=nd, trailing_empty=40, empty_run=10, masks_with_holes=True)
    return out


_CYCLE = (1, 2, 3, 4, 5, 6, 7, 8, 0)                                 # every remainder of the four-blocks-at-a-time row sum, and the empty block-row
_BLOCK_BCOLS = 300
_TAKEN_AS = {2: 2, 3: 3, 4: 2}                                       # the block size a matrix of aligned b×b blocks settles on (BCSR_ORDER)


def _main_blocks(b, at_limit):
    """3 leading empty block-rows, 10 cycles, one block-row of `at_limit` blocks, 10 cycles whose last block-row is empty and 599 more empty ones
    (600 in a row: more than one work item may hold), 50 cycles, the last one's empty block-row and one more (2 trailing): 1 234 block-rows,
    2 520 + at_limit blocks (≥ 2 per block-row on average)."""
    return [0] * 3 + list(_CYCLE) * 10 + [at_limit] + list(_CYCLE) * 10 + [0] * 599 + list(_CYCLE) * 50 + [0]


def block_cases():
    out = []
    add = lambda name, make, path, **claims: out.append(Case(name, make, path, claims))
    for b in (2, 3, 4):
        t = tile_blocks(b)
        # aligned 4×4 blocks pass the 2×2 check, which comes first: a 4×4 matrix runs as twice as many 2×2 blocks (64 → 128 per block-row at the limit)
        add(f"main_b{b}", functools.partial(block_matrix, b, _main_blocks(b, t), _BLOCK_BCOLS, seed=500 + b), PATH_BLOCKROW, block=_TAKEN_AS[b], max_blocks=t,
            mod4={0, 1, 2, 3}, empty_brow_run=600, leading_empty=3, trailing_empty_brows=2)
    # one block past the tile: b = 2 and 3 fall back to the CSR kernel; 65 aligned 4×4 blocks are 130 aligned 2×2 blocks, inside THAT tile (256):
    # the 2×2 form takes them. 129 4×4 blocks (258 2×2 blocks) are past both.
    add("over_b2", functools.partial(block_matrix, 2, _main_blocks(2, 257), _BLOCK_BCOLS, seed=512), PATH_STREAM, block=0, max_blocks=257)
    add("over_b3", functools.partial(block_matrix, 3, _main_blocks(3, 114), _BLOCK_BCOLS, seed=513), PATH_STREAM, block=0, max_blocks=114)
    add("over_b4", functools.partial(block_matrix, 4, _main_blocks(4, 65), _BLOCK_BCOLS, seed=514), PATH_BLOCKROW, block=2, max_blocks=65)
    add("over_b4_and_b2", functools.partial(block_matrix, 4, _main_blocks(4, 129), _BLOCK_BCOLS, seed=515), PATH_STREAM, block=0, max_blocks=129)
    # gates
    add("gate_rows_60", functools.partial(block_matrix, 3, [3] * 20, 20, seed=520), PATH_STREAM, block=0, rows=60)
    add("gate_rows_66", functools.partial(block_matrix, 3, [3] * 22, 22, seed=520), PATH_BLOCKROW, block=3, rows=66)
    for b in (2, 3, 4):
        add(f"gate_nnz_at_b{b}", functools.partial(block_matrix, b, [2] * 100, 100, seed=530 + b), PATH_BLOCKROW, block=_TAKEN_AS[b], nnz=2 * b * 100 * b)
        # one block short of two per block-row: b = 2 and 3 are refused; 4×4 blocks still hold two 2×2 blocks per 2×2 block-row and more
        add(f"gate_nnz_below_b{b}", functools.partial(block_matrix, b, [2] * 57 + [1] + [2] * 42, 100, seed=530 + b), PATH_BLOCKROW if b == 4 else PATH_STREAM,
            block=2 if b == 4 else 0, nnz=2 * b * 100 * b - b * b)
    add("gate_rows_mod_b", functools.partial(block_matrix, 3, [3] * 40, 40, rows_extra=1, seed=540), PATH_STREAM, block=0, rows=121)
    add("gate_cols_mod_b", functools.partial(block_matrix, 3, [3] * 40, 40, cols_extra=1, seed=541), PATH_STREAM, block=0, cols=121)
    add("gate_shift_run", functools.partial(block_matrix, 3, [3] * 40, 40, shift_run=(17, 1), seed=542), PATH_STREAM, block=0, misaligned_brow=17)
    add("gate_descending", functools.partial(block_matrix, 3, [3] * 40, 40, descending=(17,), seed=543), PATH_STREAM, block=0, descending_brow=17, unsorted=True)
    add("rect_cols_2rows", functools.partial(block_matrix, 3, [3, 2, 4, 0, 5] * 8, 80, seed=544), PATH_BLOCKROW, block=3, rows=120, cols=240)
    return out


@functools.lru_cache(maxsize=None)
def _all_cases():
    return {c.name: c for c in dia_cases() + block_cases()}


@functools.lru_cache(maxsize=None)
def build(name):
    """The arrays of a case by name, built once per process (read-only: copy before changing them)."""
    m = _all_cases()[name].make()
    for a in (m.rowptr, m.colids, m.values):
        a.setflags(write=False)
    return m


def case(name):
    return _all_cases()[name]
