"""The blocked SpMV path (g4s_amd/csrc/spmv_pb.hip, spmv_path 1) restated in numpy — the plan pb_build must produce, the product computed through
that layout, the locality probe pb_should_use — plus inputs that sit ON the edges of its plan builder and of its two kernels: degenerate shapes,
empty row and column bands, the hot-band decision at its threshold, rank ties, colliding slots of the degree hash, producer items of exactly one
STEP / k·STEP + one window / one window, consumer items of 4 / 8 192 / 8 196 / 2·8 192 + 4 slots, and a hub row at local row 0 that fills whole
waves of a consumer item. numpy only: no GPU, no torch.

tests/test_pb_cases_cpu.py proves that every case reaches the edge its name claims, that the union covers every edge, and that the modelled layout
is a valid plan (emulate equals a long-double product); tests/test_spmv_pb_limits_gpu.py holds the device to the model (the plan's debug line,
field by field) and to the oracle.

The one edge left to the full-size configuration test (tests/test_configs_gpu.py): the BINNED degree count (pb_bin_keys_kernel /
pb_bin_degree_kernel) is reached only from cols >= 2^20 with nnz >= 2^24 — too large for a test that takes seconds. Every case here counts its
degrees with pb_col_degree_kernel's hashed LDS table. The int32 overflow guards of pb_build cannot be reached at these sizes either."""
import functools
from typing import Callable, NamedTuple, Optional

import numpy as np

# ---- the plan's constants, each beside the source line of spmv_pb.hip it mirrors
BAND_WIDE = 20448            # `constexpr int kBandWide = 20448;` — where a workgroup may have 160 KiB of LDS
BAND_NARROW = 16384          # `constexpr int kBandNarrow = 16384;` — otherwise, or with G4S_PB_BAND=16384
SPAN = 8                     # `constexpr int kSpan = 8;` — cells are padded to a multiple of it
WINDOW = 32                  # `constexpr int kWindow = 32;` — column bands start at multiples of it; a micro-run never crosses one
MAX_HOT_BANDS = 64           # `constexpr int kMaxHotBands = 64;` — `const int Hmax = std::min(kMaxHotBands, cols / (2 * W));`
HOT_FACTOR = 4.0             # `constexpr double kHotFactor = 4.0;` — `if ((double)in_band < kHotFactor * avg) break;`, avg = (double)nnz / CBnat
PB_THREADS = 1024            # `constexpr int kPbThreads = 1024;`
PAIR_UNROLL = 4              # `#define G4S_PB_PAIR_UNROLL 4` — producer: `constexpr int STEP = kPbThreads * kPairUnroll;` PAIRS of entries per trip
CONS_UNROLL = 2              # `#define G4S_PB_CONS_UNROLL 2` — consumer: `constexpr int STEP = 4 * kPbThreads * kPbUnroll;` slots per trip
PRODUCER_STEP = 2 * PB_THREADS * PAIR_UNROLL    # 8 192 entries per trip of a producer workgroup
CONSUMER_STEP = 4 * PB_THREADS * CONS_UNROLL    # 8 192 slots per trip of a consumer workgroup
PRODUCER_CHUNK = 1 << 17     # `constexpr int kProducerChunk = 1 << 17;`
CONSUMER_CHUNK = 1 << 17     # `constexpr int kConsumerChunk = 1 << 17;`
AUTO_PC_FLOOR = 32768        # `auto_pc = std::min<long long>(kProducerChunk, std::max<long long>(32768, pow2_at_most(totP / 128)));`
AUTO_CC_FLOOR = 16384        # `auto_cc = std::min<long long>(kConsumerChunk, std::max<long long>(16384, pow2_at_most(P->micro_runs / 128)));`
PCHUNK_FLOOR = SPAN * PB_THREADS   # `kPC = (std::max<long long>(kSpan * kPbThreads, G4S_PB_PCHUNK or auto_pc) / kWindow) * (kWindow / kSpan);` spans, whole windows
CCHUNK_FLOOR = 4             # `kCC = (int)std::max<long long>(4, (G4S_PB_CCHUNK or auto_cc) & ~3ll);`
DEG_SLOTS = 4096             # `constexpr int kDegSlots = 4096, kDegBlocks = 2048;`
DEG_BLOCKS = 2048            # grid of pb_col_degree_kernel: `std::min<long long>(kDegBlocks, (nnz + 255) / 256)`
DEG_HASH_MUL = 2654435761    # pb_col_degree_kernel: `const int h = (int)(((unsigned)c * 2654435761u) >> 20);`
BIN_MIN_COLS = 1 << 20       # pb_build: `if (cols >= (1 << 20) && nnz >= (1ll << 24) && …)` → the binned degree count (not reached here)
BIN_MIN_NNZ = 1 << 24
# ---- pb_should_use
PB_MIN_X_BYTES = 8 << 20     # `if ((long long)cols * 8 < (8ll << 20) || nnz < (4ll << 20)) return false;`
PB_MIN_NNZ = 4 << 20         # (the same line)
PROBE_WINDOW = 2048          # `const int W = 2048, S = 16;` — S windows of W consecutive column ids, window w from position w·((nnz − W) / S) on
PROBE_SAMPLES = 16
PROBE_LINE_SHIFT = 4         # `h[i] >>= 4;` — sixteen doubles to a 128-byte line of x
PROBE_RATIO = 0.5            # `return ratio / S > 0.5;` — ratio = Σ distinct lines of a window / W
PATH_STREAM, PATH_BLOCKED = 0, 1

INT_MAX_ABS = 7              # integer-valued data: |value|, |x| <= 7 and |y0| <= 1000 (see integer_data)
INT_Y_MAX_ABS = 1000


def pow2_at_most(v):
    """pb_build: `auto pow2_at_most = [](long long v) { long long p = 1; while (p * 2 <= v) p *= 2; return p; };`"""
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def deg_hash(c):
    """The slot of column c in pb_col_degree_kernel's LDS table (12 bits)."""
    return ((np.asarray(c, np.uint64) * np.uint64(DEG_HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)


def deg_block_shares(nnz):
    """[k0, k1) of every workgroup of pb_col_degree_kernel: `per = (nnz + gridDim.x − 1) / gridDim.x, k0 = per * blockIdx.x`."""
    grid = min(DEG_BLOCKS, (nnz + 255) // 256)
    per = (nnz + grid - 1) // grid
    return [(b * per, min(nnz, b * per + per)) for b in range(grid) if b * per < nnz]


class Plan(NamedTuple):
    rows: int
    cols: int
    W: int
    H: int
    Hmax: int
    CBnat: int
    CB: int
    RB: int
    nnz: int
    hot_cols: np.ndarray     # the H·W hot columns in rank order (pb_colmap_hot_kernel)
    col_band: np.ndarray     # colmap[col] >> 15
    col_local: np.ndarray    # colmap[col] & 0x7FFF
    in_band: list            # entries of each ranked band the automatic rule looked at (empty when H was forced or Hmax == 0)
    cell_start: np.ndarray   # padP: padded position of every cell q = c·RB + r, and the padded length behind the last
    padded: int
    pos: np.ndarray          # padded producer position of CSR entry k
    p_row: np.ndarray        # row at every padded position, −1 = pad
    p_src: np.ndarray        # CSR index at every padded position, −1 = pad
    p_band: np.ndarray       # column band of every padded position (pads: the band whose span range holds them)
    p_local: np.ndarray      # local column at every padded position, W = pad (the zero word)
    head: np.ndarray         # bool per padded position: opens a micro-run
    micro_runs: int
    run_slot: np.ndarray     # consumer slot of every micro-run, in producer order
    c_lrow: np.ndarray       # local row of every consumer slot (pads: 0)
    band_start: np.ndarray   # bandC: RB + 1 multiples of 4
    band_end: np.ndarray     # bandE: the first pad slot of each row band
    kPC: int                 # spans per producer item
    kCC: int                 # slots per consumer item of a split band
    pitems: list             # (cband, s0, s1) spans, heaviest first
    citems: list             # (rband, k0, k1, split), heaviest first
    split: list              # the split row bands

    def debug_fields(self):
        """The fields of pb_build's G4S_DEBUG line, in its order: band, CB, RB, hot, nnz, padded, micro-runs, producer items, consumer items, split bands."""
        return (self.W, self.CB, self.RB, self.H, self.nnz, self.padded, self.micro_runs, len(self.pitems), len(self.citems), len(self.split))


def row_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr).astype(np.int64))


def rank_columns(colids, cols, ties="ascending"):
    """Column degrees and the columns by descending degree; equal degrees keep ascending column ids (pb_build sorts (deg, iota) with the library's
    STABLE descending radix sort). ties="descending" is the wrong order, for the tests that prove a case notices it."""
    deg = np.bincount(np.asarray(colids, np.int64), minlength=cols)
    ids = np.arange(cols, dtype=np.int64)
    return deg, np.lexsort((ids if ties == "ascending" else -ids, -deg))


def plan(rowptr, colids, rows, cols, W, hot=None, pchunk=None, cchunk=None, ties="ascending", deg=None):
    """What pb_build must produce for this matrix at band width W. hot / pchunk / cchunk: G4S_PB_HOT_BANDS / G4S_PB_PCHUNK / G4S_PB_CCHUNK (None: unset).
    deg: other column degrees than the true ones (for the tests that prove a case notices a miscount)."""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colids, np.int64)
    nnz = int(rp[-1])
    assert nnz > 0 and rows > 0 and cols > 0 and len(ci) == nnz
    # 0. hot column bands
    CBnat = (cols + W - 1) // W
    Hmax = min(MAX_HOT_BANDS, cols // (2 * W))
    H, in_band, order = 0, [], np.zeros(0, np.int64)
    want = -1 if hot is None else int(hot)                              # `const int want = e ? atoi(e) : -1;`
    if want != 0 and Hmax > 0:
        true_deg, order = rank_columns(ci, cols, ties)
        if deg is not None:
            ids = np.arange(cols, dtype=np.int64)
            order = np.lexsort((ids if ties == "ascending" else -ids, -np.asarray(deg, np.int64)))
        ranked = (true_deg if deg is None else np.asarray(deg, np.int64))[order]
        if want > 0:
            H = min(want, Hmax)
        else:
            avg = float(nnz) / CBnat
            for h in range(Hmax):
                n = int(ranked[h * W:(h + 1) * W].sum())
                in_band.append(n)
                if float(n) < HOT_FACTOR * avg:
                    break
                H = h + 1
    CB, RB = CBnat + H, (rows + W - 1) // W
    col_band = np.arange(cols, dtype=np.int64) // W + H
    col_local = np.arange(cols, dtype=np.int64) % W
    hot_cols = order[:H * W].copy()
    col_band[hot_cols] = np.arange(H * W) // W
    col_local[hot_cols] = np.arange(H * W) % W
    # 1. regroup: a stable sort by (column band, row band)
    row = row_of(rp)
    cell = col_band[ci] * RB + row // W
    perm = np.argsort(cell, kind="stable")
    ncells = CB * RB
    start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=ncells))])
    # 2. padded producer layout: a column band starts on a window, a cell on a span
    cell_start, shift, tot = np.zeros(ncells + 1, np.int64), np.zeros(ncells, np.int64), 0
    for q in range(ncells):
        if q % RB == 0:
            tot = -(-tot // WINDOW) * WINDOW
        cell_start[q], shift[q] = tot, tot - start[q]
        tot = -(-(tot + start[q + 1] - start[q]) // SPAN) * SPAN
    tot = -(-tot // WINDOW) * WINDOW
    cell_start[ncells] = padded = int(tot)
    scell = cell[perm]
    spos = np.arange(nnz, dtype=np.int64) + shift[scell]
    pos = np.empty(nnz, np.int64)
    pos[perm] = spos
    p_row, p_src, p_cell = np.full(padded, -1, np.int64), np.full(padded, -1, np.int64), np.full(padded, -1, np.int64)
    p_local = np.full(padded, W, np.int64)
    p_row[spos], p_src[spos], p_cell[spos], p_local[spos] = row[perm], perm, scell, col_local[ci[perm]]
    band_first = cell_start[np.arange(CB + 1) * RB]                      # padded position where each column band starts
    p_band = np.searchsorted(band_first, np.arange(padded), side="right") - 1
    # 3. micro-run heads: a real entry that opens its cell or its window, or whose row differs from the previous entry's
    real = p_row >= 0
    head = real.copy()
    cont = real[1:] & real[:-1] & (p_cell[1:] == p_cell[:-1]) & (p_row[1:] == p_row[:-1]) & (np.arange(1, padded) % WINDOW != 0)
    head[1:] &= ~cont
    heads_before = np.concatenate([[0], np.cumsum(head)])
    micro_runs = int(heads_before[-1])
    mstart = heads_before[cell_start]                                    # micro-run index at every cell start
    # 4. consumer layout: the cells of a row band one after the other (by column band), bands at multiples of 4
    delta, band_start, band_end, totc = np.zeros(ncells, np.int64), np.zeros(RB + 1, np.int64), np.zeros(RB, np.int64), 0
    for r in range(RB):
        totc = (totc + 3) & ~3
        band_start[r] = totc
        for c in range(CB):
            q = c * RB + r
            delta[q] = totc - mstart[q]
            totc += mstart[q + 1] - mstart[q]
        band_end[r] = totc
    totc = (totc + 3) & ~3
    band_start[RB] = totc
    head_pos = np.flatnonzero(head)
    run_slot = np.arange(micro_runs, dtype=np.int64) + delta[p_cell[head_pos]]
    c_lrow = np.zeros(totc, np.int64)
    c_lrow[run_slot] = p_row[head_pos] % W
    # 5. work items, heaviest first (stable)
    auto_pc = min(PRODUCER_CHUNK, max(AUTO_PC_FLOOR, pow2_at_most(padded // 128)))
    auto_cc = min(CONSUMER_CHUNK, max(AUTO_CC_FLOOR, pow2_at_most(micro_runs // 128)))
    kPC = (max(PCHUNK_FLOOR, auto_pc if pchunk is None else int(pchunk)) // WINDOW) * (WINDOW // SPAN)
    kCC = max(CCHUNK_FLOOR, (auto_cc if cchunk is None else int(cchunk)) & ~3)
    pitems = []
    for c in range(CB):
        s0, s1 = int(band_first[c]) // SPAN, int(band_first[c + 1]) // SPAN
        pitems += [(c, s, min(s1, s + kPC)) for s in range(s0, s1, kPC)]
    citems, split = [], []
    for r in range(RB):
        b0, b1 = int(band_start[r]), int(band_start[r + 1])
        if b1 - b0 <= kCC:
            citems.append((r, b0, b1, 0))                                # also the empty bands: their rows must still be written
        else:
            split.append(r)
            citems += [(r, k, min(b1, k + kCC), 1) for k in range(b0, b1, kCC)]
    pitems.sort(key=lambda it: -(it[2] - it[1]))
    citems.sort(key=lambda it: -(it[2] - it[1]))
    return Plan(rows, cols, W, H, Hmax, CBnat, CB, RB, nnz, hot_cols, col_band, col_local, in_band, cell_start, padded, pos, p_row, p_src, p_band, p_local, head,
                micro_runs, run_slot, c_lrow, band_start, band_end, kPC, kCC, pitems, citems, split)


def emulate(P, values, x, alpha=1.0, beta=0.0, y0=None):
    """y = alpha·A·x + beta·y0 computed THROUGH the modelled layout, in numpy long double: hot x gathered, every producer item reads its band of x (zeros
    past the last column, the zero word for pads) and sums its micro-runs, every consumer item folds its slots into its row band; split bands start
    from beta·y0 and add, the others are written once. y starts as NaN: a row no item writes stays NaN. Asserts that the items tile the layout."""
    ld = np.longdouble
    W, H, rows, cols = P.W, P.H, P.rows, P.cols
    x = np.asarray(x, ld)
    assert len(x) == cols
    hot_x = x[P.hot_cols]                                                # pb_prepare_kernel: hot_x[r] = x[hot_cols[r]]
    p_val = np.zeros(P.padded, ld)
    p_val[P.p_src >= 0] = np.asarray(values, ld)[P.p_src[P.p_src >= 0]]
    sums, seen = np.zeros(P.micro_runs, ld), np.zeros(P.padded, np.int64)
    run_of = np.cumsum(P.head) - 1
    for c, s0, s1 in P.pitems:
        a, b = s0 * SPAN, s1 * SPAN
        assert np.all(P.p_band[a:b] == c) and a % WINDOW == 0
        seen[a:b] += 1
        xs = np.zeros(W + 1, ld)                                         # the band of x and the zero word
        src, c0, limit = (hot_x, c * W, H * W) if c < H else (x, (c - H) * W, cols)
        n = max(0, min(W, limit - c0))
        xs[:n] = src[c0:c0 + n]
        prod = p_val[a:b] * xs[P.p_local[a:b]]
        live = P.p_row[a:b] >= 0
        assert np.all(prod[~live] == 0)
        np.add.at(sums, run_of[a:b][live], prod[live])
    assert np.all(seen[P.p_row >= 0] == 1) and seen.max(initial=0) <= 1, "the producer items do not tile the entries"
    slot_val = np.zeros(len(P.c_lrow), ld)
    slot_val[P.run_slot] = sums
    y = np.full(rows, np.nan, ld)
    y0 = np.zeros(rows, ld) if y0 is None else np.asarray(y0, ld)
    for r in P.split:                                                    # pb_prepare_kernel
        a, b = r * W, min(rows, (r + 1) * W)
        y[a:b] = 0.0 if beta == 0.0 else ld(beta) * y0[a:b]
    covered = np.zeros(len(P.c_lrow), np.int64)
    for r, k0, k1, is_split in P.citems:
        assert k0 % 4 == 0 and k1 % 4 == 0 and P.band_start[r] <= k0 <= k1 <= P.band_start[r + 1]
        covered[k0:k1] += 1
        ys = np.zeros(W, ld)
        np.add.at(ys, P.c_lrow[k0:k1], slot_val[k0:k1])
        a, b = r * W, min(rows, (r + 1) * W)
        assert np.all(ys[b - a:] == 0), "a slot points past the last row"
        if is_split:
            y[a:b] += ld(alpha) * ys[:b - a]
        else:
            y[a:b] = ld(alpha) * ys[:b - a] + (0.0 if beta == 0.0 else ld(beta) * y0[a:b])
    assert np.all(covered == 1), "the consumer items do not tile the slots"
    return y


def wave_branches(P, item):
    """(wave-uniform, per-lane) counts of the 256-slot wave turns of a consumer item: a wavefront takes 64 groups of 4 consecutive slots per turn, and
    the uniform branch needs all 64 groups inside the item and all 256 slots on one local row (`__all(active && lane_uniform && r0_ == first_row)`)."""
    _, k0, k1, _ = item
    uniform = mixed = 0
    for a in range(k0, k1, 256):
        rows_ = P.c_lrow[a:min(a + 256, k1)]
        if a + 256 <= k1 and np.all(rows_ == rows_[0]):
            uniform += 1
        else:
            mixed += 1
    return uniform, mixed


def tail_wave_on_one_row(P, item):
    """The last wave turn of the item holds fewer than 64 groups and all its slots, pads included, name one local row: the lanes past the end must
    count as inactive there (they once left the loop, and the wave-uniform branch shuffled from them)."""
    _, k0, k1, _ = item
    tail = P.c_lrow[k1 - (k1 - k0) % 256:k1]
    return 0 < len(tail) < 256 and bool(np.all(tail == tail[0]))


def should_use(rows, cols, nnz, colids):
    """pb_should_use: (decision, ratio); the ratio is None where the size gates decide. The sum of the window ratios is a multiple of 1/2048 below 16
    and its sixteenth is exact in fp64, so the decision is exact: blocked if and only if the windows hold more than 16 384 distinct lines in all."""
    if cols * 8 < PB_MIN_X_BYTES or nnz < PB_MIN_NNZ:
        return False, None
    stride = (nnz - PROBE_WINDOW) // PROBE_SAMPLES
    ratio = 0.0
    for w in range(PROBE_SAMPLES):
        lines = np.asarray(colids[w * stride:w * stride + PROBE_WINDOW], np.int64) >> PROBE_LINE_SHIFT
        ratio += len(np.unique(lines)) / PROBE_WINDOW
    ratio /= PROBE_SAMPLES
    return ratio > PROBE_RATIO, ratio


# ------------------------------------------------------------------------------------------------ matrices
class Matrix(NamedTuple):
    rowptr: np.ndarray       # int32
    colids: np.ndarray       # int32, ascending and distinct inside a row
    values: np.ndarray       # float64, U(−1, 1)
    rows: int
    cols: int
    x: np.ndarray            # float64, U(−1, 1)
    y0: np.ndarray           # float64, U(−1, 1)
    ivalues: np.ndarray      # float64 holding integers of [−7, 7] without 0
    ix: np.ndarray           # float64 holding integers of [−7, 7]
    iy0: np.ndarray          # float64 holding integers of [−1000, 1000]


def integer_data(rowptr, cols, rng):
    """Integer-valued values, x and y0 for the bit-for-bit checks. With |value|, |x| <= 7 and |y0| <= 1000 every partial sum of a row of L entries —
    in any order, the old y included — is an integer of magnitude <= 49·L + 1000. While that stays below 2^53 every such integer is an fp64 number and
    every addition is exact, so the result does not depend on the order of the LDS atomics."""
    lens = np.diff(np.asarray(rowptr, np.int64))
    rows = len(lens)
    assert INT_MAX_ABS * INT_MAX_ABS * int(lens.max(initial=0)) + INT_Y_MAX_ABS < 2 ** 53
    nnz = int(lens.sum())
    iv = rng.integers(1, INT_MAX_ABS + 1, nnz) * rng.choice([-1, 1], nnz)
    ix = rng.integers(-INT_MAX_ABS, INT_MAX_ABS + 1, cols)
    iy0 = rng.integers(-INT_Y_MAX_ABS, INT_Y_MAX_ABS + 1, rows)
    return iv.astype(np.float64), ix.astype(np.float64), iy0.astype(np.float64)


def from_pairs(rows, cols, r, c, seed):
    """The CSR matrix of the (row, column) pairs, which must be distinct; rows sorted by column."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    assert r.size and r.min() >= 0 and r.max() < rows and c.min() >= 0 and c.max() < cols
    key = np.sort(r * cols + c)
    assert np.all(np.diff(key) > 0), "a (row, column) pair repeats"
    rp = np.zeros(rows + 1, np.int64)
    np.add.at(rp, key // cols + 1, 1)
    rng = np.random.default_rng(seed)
    rp = np.cumsum(rp)
    va, x, y0 = rng.uniform(-1, 1, key.size), rng.uniform(-1, 1, cols), rng.uniform(-1, 1, rows)
    iv, ix, iy0 = integer_data(rp, cols, rng)
    return Matrix(rp.astype(np.int32), (key % cols).astype(np.int32), va, int(rows), int(cols), x, y0, iv, ix, iy0)


def _cat(*pairs):
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def _fill(n, row0, nrows, col0, width):
    """n entries in columns [col0, col0 + width) spread level over rows [row0, row0 + nrows): ⌈n / nrows⌉ to a row, evenly spaced columns."""
    per = -(-n // nrows)
    assert 0 < per <= width
    e = np.arange(n, dtype=np.int64)
    return row0 + e // per, col0 + (e % per) * (width // per)


def _scatter(cols):
    """Column ids in a scattered order: a permutation of [0, cols)."""
    assert cols % 7919 != 0
    return (np.arange(cols, dtype=np.int64) * 7919) % cols


# ---- shapes
def _one_by_one(W):
    return from_pairs(1, 1, [0], [0], 1)


def _one_row(W):
    cols = 2 * W + 40
    return from_pairs(1, cols, np.zeros(cols, np.int64), np.arange(cols), 2)


def _one_col(W):
    rows = 2 * W + 40
    return from_pairs(rows, 1, np.arange(rows), np.zeros(rows, np.int64), 3)


def _small(W):
    r = np.repeat(np.arange(300), 7)
    c = (r * 13 + np.tile(np.arange(7), 300) * 29) % 200
    return from_pairs(300, 200, r, c, 4)


def _cols_edge(W, cols):
    """Three entries to a row over W + 300 rows; the last row and the last column hold an entry."""
    rows = W + 300
    r = np.repeat(np.arange(rows - 1), 3)
    c = (r * 7919 + np.tile(np.arange(3), rows - 1) * (cols // 3)) % cols
    return from_pairs(rows, cols, np.append(r, rows - 1), np.append(c, cols - 1), 5)


def _empty_row_bands(W):
    """Four row bands; bands 1 (in the middle) and 3 (the last, 50 rows) hold no entry."""
    rows, cols = 3 * W + 50, W + 500
    r = np.concatenate([np.arange(0, W, 5), np.arange(2 * W, 3 * W, 5)])
    r3 = np.repeat(r, 3)
    c = (r3 * 31 + np.tile(np.arange(3), len(r)) * (cols // 3)) % cols
    return from_pairs(rows, cols, r3, c, 6)


def _empty_col_bands(W):
    """Four natural column bands; bands 1 (in the middle) and 3 (the last, 50 columns) hold no entry."""
    rows, cols = W + 100, 3 * W + 50
    r = np.repeat(np.arange(rows), 2)
    c = np.where(np.tile([0, 1], rows) == 0, (r * 37) % W, 2 * W + (r * 41) % W)
    return from_pairs(rows, cols, r, c, 7)


# ---- hot bands
def _profile(W, cols, groups, cold, seed, moved=0, rows=None):
    """Column degrees by group: groups = [(columns, degree), …] in scattered column order, then `cold` columns of degree 1. moved: that many entries
    of the first group's last column go to fresh cold columns instead."""
    rows = 2 * W + 9 if rows is None else rows
    ids = _scatter(cols)
    dmax = max(d for _, d in groups)
    rr, cc, at = [], [], 0
    for n, d in list(groups) + [(cold, 1)]:
        i = np.repeat(np.arange(at, at + n), d)
        t = np.tile(np.arange(d), n)
        rr.append((i * 3 + t * (rows // dmax)) % rows)
        cc.append(ids[i])
        at += n
    r, c = np.concatenate(rr), np.concatenate(cc)
    if moved:
        last = np.flatnonzero(c == ids[groups[0][0] - 1])[:moved]
        assert len(last) == moved and at + moved <= cols
        c[last] = ids[at:at + moved]
    return from_pairs(rows, cols, r, c, seed)


def _hot_exact(W, moved=0):
    """8 natural bands, nnz = 8·W: W columns of degree 4 (the first ranked band: 4·W entries = kHotFactor · nnz / 8 exactly) and 4·W of degree 1."""
    return _profile(W, 8 * W, [(W, 4)], 4 * W, 8, moved=moved)


def _hot_two_of_four(W):
    """10 natural bands (Hmax 4), nnz = 10·W: ranked bands of 5·W, 4·W (= kHotFactor · nnz / 10 exactly) and W entries: the rule stops at H = 2."""
    return _profile(W, 9 * W + 100, [(W, 5), (W, 4)], W, 9)


TIE_EXTRA = 99               # columns of the tied degree beyond the W that fit the hot band


def _hot_tie(W):
    """W + 99 columns of degree 2 and one hot band (forced): the W lowest ids are hot. The 99 lowest keep both entries in row band 0, the 99 highest
    (the losers) both in row band 1, the others one in each — another tie order moves 198 entries between the cells of the hot band."""
    rows, cols = 2 * W, 4 * W + 77
    tied = np.sort(_scatter(cols)[:W + TIE_EXTRA])
    i = np.arange(W + TIE_EXTRA)
    first = np.where(i >= W, W, 0) + (i * 5) % W                       # the losers' first entry: row band 1
    second = np.where(i < TIE_EXTRA, 0, W) + (i * 5 + 1) % W            # the lowest ids' second entry: row band 0
    cold = _scatter(cols)[W + TIE_EXTRA:2 * W]
    return from_pairs(rows, cols, np.concatenate([first, second, (np.arange(len(cold)) * 2) % rows]), np.concatenate([tied, tied, cold]), 10)


HASH_POPULAR, HASH_DEGREE, HASH_SLOTS = 120, 600, 5


def hash_popular_columns(W):
    """120 columns of [0, 8·W) whose ids fall into five slots of pb_col_degree_kernel's table (at least 16 to a slot)."""
    c = np.arange(8 * W, dtype=np.int64)
    h = deg_hash(c)
    pop = c[h < HASH_SLOTS][:HASH_POPULAR]                               # the columns of the first five slots, about 8·W / 4 096 to a slot
    assert len(pop) == HASH_POPULAR and np.bincount(h[pop].astype(np.int64)).min() >= 16
    return pop


def _deg_hash(W, moved=0):
    """120 popular columns of degree 600 in five slots of the degree hash (16 or more to a slot), and cold columns of degree 1 — as many as put the first
    ranked band (the popular columns and W − 120 cold ones) at exactly kHotFactor · nnz / 8 entries: H must be 1 (moved: one entry short, H 0).
    Neighbouring rows hold different popular columns, so a workgroup's share of the entries holds many columns of one slot: one is counted in LDS,
    the others in HBM, and another workgroup may choose another owner."""
    cols, rows = 8 * W, 2 * W + 9
    pop = hash_popular_columns(W)
    ncold = HASH_POPULAR * HASH_DEGREE + 2 * W - 2 * HASH_POPULAR
    rest = np.setdiff1d(_scatter(cols), pop, assume_unique=True)         # (sorted by setdiff1d)
    cold = rest[np.linspace(0, len(rest) - 1, ncold + 1).astype(np.int64)]   # spread over all natural bands; one more than needed, for `moved`
    assert len(np.unique(cold)) == ncold + 1
    j = np.repeat(np.arange(HASH_POPULAR), HASH_DEGREE)
    t = np.tile(np.arange(HASH_DEGREE), HASH_POPULAR)
    r, c = (t * HASH_POPULAR + j) % rows, pop[j]
    if moved:
        c = c.copy()
        c[-1] = cold[ncold]
    rc, cc = (np.arange(ncold) * 11) % rows, cold[:ncold]
    return from_pairs(rows, cols, np.concatenate([r, rc]), np.concatenate([c, cc]), 11)


# ---- producer items: 600 rows (one row band), three column bands (the last 100 columns wide), no hot band: a band's padded length is its entry count
# rounded up to a window
P_ROWS = 600


def _producer(W, n0, n1, n2=40):
    return from_pairs(P_ROWS, 2 * W + 100, *_cat(_fill(n0, 0, P_ROWS, 0, W), _fill(n1, 0, P_ROWS, W, W), _fill(n2, 0, P_ROWS, 2 * W, 100)), 12)


def _producer_hub(W):
    """Row 300 holds every column of band 0, rows 100 and 500 ten entries of it each: the hub's run crosses every item boundary of the band."""
    few = np.arange(10) * 50
    return from_pairs(P_ROWS, 2 * W + 100, *_cat((np.full(10, 100), few), (np.full(W, 300), np.arange(W)), (np.full(10, 500), few + 7),
                                                  _fill(3000, 0, P_ROWS, W, W), _fill(40, 0, P_ROWS, 2 * W, 100)), 13)


# ---- consumer items
C_RUNS = 3 * (2 * CONSUMER_STEP + 4)   # 49 164 micro-runs in row band 0: 6 items of 8 192 + 12, 5 of 8 196 + 8 184, 3 of 16 388


def _consumer(W):
    """Four column bands, no hot band. Rows 0 … 12 290 hold one entry in each column band (four micro-runs each: 49 164 in row band 0), the 1 000 rows
    of row band 1 one entry each."""
    n = C_RUNS // 4
    r = np.repeat(np.arange(n), 4)
    b = np.tile(np.arange(4), n)
    r1 = W + np.arange(1000)
    return from_pairs(W + 1000, 4 * W, np.concatenate([r, r1]), np.concatenate([b * W + (r * 17 + b * 5) % W, (r1 * 29) % (4 * W)]), 14)


def _consumer_wave(W):
    """Row W — local row 0 of row band 1, the row the pad slots name — holds every column of band 0: its W entries are ⌈W / 32⌉ micro-runs or one more
    (row 3's eight entries put the cell off the window grid), consecutive slots at the start of the band's one item: two whole waves of 256 slots
    and a wave the run ends in. 599 more rows of three entries follow."""
    rows, cols = W + 600, W + 64
    r = np.repeat(W + 1 + np.arange(599), 3)
    c = (r * 53 + np.tile(np.arange(3), 599) * (cols // 3)) % cols
    return from_pairs(rows, cols, *_cat((np.full(8, 3), np.arange(8) * 9), (np.full(W, W), np.arange(W)), (r, c)), 15)


class Case(NamedTuple):
    name: str
    group: str               # shapes / hot / producer / consumer
    make: Callable[[int], Matrix]
    hot: Optional[int]       # G4S_PB_HOT_BANDS (None: unset, the automatic rule)
    pchunk: Optional[int]    # G4S_PB_PCHUNK
    cchunk: Optional[int]    # G4S_PB_CCHUNK
    claims: dict             # what tests/test_pb_cases_cpu.py proves about it


def _cases():
    out = []
    add = lambda name, group, make, hot=None, pchunk=None, cchunk=None, **claims: out.append(Case(name, group, make, hot, pchunk, cchunk, claims))
    add("one_by_one", "shapes", _one_by_one, shape=(1, 1), bands=(1, 1), tail_wave_on_one_row=True)
    add("one_row", "shapes", _one_row, rows=1, every_column=True, hub_local_row0=True)
    add("one_col", "shapes", _one_col, cols=1, every_row=True)
    add("below_one_band", "shapes", _small, bands=(1, 1), below_band=True)
    add("cols_2w_minus_1", "shapes", lambda W: _cols_edge(W, 2 * W - 1), Hmax=0, H=0)
    add("cols_2w", "shapes", lambda W: _cols_edge(W, 2 * W), Hmax=1, H=0, ranked=True)
    add("cols_2w_minus_1_hot_asked", "shapes", lambda W: _cols_edge(W, 2 * W - 1), hot=3, Hmax=0, H=0)
    add("cols_2w_hot_asked", "shapes", lambda W: _cols_edge(W, 2 * W), hot=64, Hmax=1, H=1, clamped=True)
    add("empty_row_bands", "shapes", _empty_row_bands, empty_row_bands=[1, 3])
    add("empty_row_bands_split", "shapes", _empty_row_bands, cchunk=2048, empty_row_bands=[1, 3], split=[0, 2])
    add("empty_col_bands", "shapes", _empty_col_bands, empty_col_bands=[1, 3], H=0)
    add("hot_exact", "hot", _hot_exact, Hmax=4, H=1, exact_band=0)
    add("hot_one_short", "hot", functools.partial(_hot_exact, moved=1), Hmax=4, H=0, short_by=1)
    add("hot_two_of_four", "hot", _hot_two_of_four, Hmax=4, H=2, exact_band=1)
    add("hot_clamped", "hot", _hot_two_of_four, hot=9, Hmax=4, H=4, clamped=True)
    add("hot_tie", "hot", _hot_tie, hot=1, Hmax=2, H=1, tie=True)
    add("deg_hash", "hot", _deg_hash, Hmax=4, H=1, exact_band=0, hash_collisions=True)
    add("deg_hash_one_short", "hot", functools.partial(_deg_hash, moved=1), Hmax=4, H=0, short_by=1, hash_collisions=True)
    S = PRODUCER_STEP
    add("p_one_step", "producer", lambda W: _producer(W, 3 * S - 3, S + 5), hot=0, pchunk=S, items=[S, S, S, S, WINDOW, 2 * WINDOW], last_window=True)
    add("p_floor", "producer", lambda W: _producer(W, 3 * S - 3, S + 5), hot=0, pchunk=1, items=[S, S, S, S, WINDOW, 2 * WINDOW], last_window=True)
    add("p_two_steps_window", "producer", lambda W: _producer(W, 2 * (2 * S + WINDOW), 2 * S + WINDOW + 20), hot=0, pchunk=2 * S + WINDOW,
        items=[2 * S + WINDOW] * 3 + [WINDOW, 2 * WINDOW], last_window=True)
    add("p_hub_row", "producer", _producer_hub, hot=0, pchunk=S, hub_row=300)
    C = CONSUMER_STEP
    add("c_items_4", "consumer", _small, cchunk=4, item_slots=4)
    add("c_floor", "consumer", _small, cchunk=1, item_slots=4)
    add("c_items_8192", "consumer", _consumer, hot=0, cchunk=C, item_slots=C, full_items=6, tail=12)
    add("c_items_8196", "consumer", _consumer, hot=0, cchunk=C + 4, item_slots=C + 4, full_items=5, tail=C_RUNS - 5 * (C + 4))
    add("c_items_16388", "consumer", _consumer, hot=0, cchunk=2 * C + 4, item_slots=2 * C + 4, full_items=3, tail=0)
    add("c_wave_uniform", "consumer", _consumer_wave, hot=0, hub_local_row0=True, uniform_waves=2)
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]
_BY_NAME = {c.name: c for c in CASES}
assert len(_BY_NAME) == len(CASES)
GROUPS = ("shapes", "hot", "producer", "consumer")
UPDATABLE_NAMES = ["empty_row_bands_split", "hot_two_of_four", "p_two_steps_window", "c_items_8196"]   # one case per edge group


def case(name):
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def build(name, W):
    """The case's matrix at band width W (cached: read-only)."""
    m = _BY_NAME[name].make(W)
    for a in m:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def model(name, W):
    """The plan pb_build must produce for the case at band width W, under the case's environment."""
    c, m = _BY_NAME[name], build(name, W)
    return plan(m.rowptr, m.colids, m.rows, m.cols, W, hot=c.hot, pchunk=c.pchunk, cchunk=c.cchunk)


# ------------------------------------------------------------------------------------------------ the automatic path: matrices the probe looks at
AUTO_ROWS, AUTO_ROW_LEN = 1 << 18, 16


def _auto_scattered(cols, nnz):
    """2^18 rows of 16 entries, one in each 65 536-column block at an offset that jumps from row to row (ids clipped to the last column): about
    sixteen distinct lines of x to a row."""
    r = np.arange(AUTO_ROWS, dtype=np.int64)
    c = np.minimum(np.arange(AUTO_ROW_LEN)[None, :] * 65536 + ((r * 40503) % 65536)[:, None], cols - 1).ravel()[:nnz]
    rp = np.minimum(np.arange(AUTO_ROWS + 1, dtype=np.int64) * AUTO_ROW_LEN, nnz)
    return rp.astype(np.int32), c.astype(np.int32)


def _auto_ratio(delta):
    """The same shape with the entries of a row in eight pairs, each pair on one line of x, no line twice within 512 neighbouring rows: every probe
    window holds exactly 1 024 lines (ratio 0.5, not blocked). delta = +1: the second entry of row 0 moves to a line of its own; −1: the second
    pair of row 0 moves onto row 1's line."""
    r = np.arange(AUTO_ROWS, dtype=np.int64)
    j = np.arange(AUTO_ROW_LEN)
    line = (j // 2)[None, :] * 8192 + ((r * 40503) % 8192)[:, None]
    c = line * 16 + (j % 2)[None, :]
    if delta > 0:
        used = set(line[:PROBE_WINDOW // AUTO_ROW_LEN, 0].tolist())
        free = next(u for u in range(1, 8192) if u not in used)
        c[0, 1] = free * 16 + 1
    elif delta < 0:
        c[0, 2:4] = line[1, 2] * 16 + np.array([2, 3])
    assert np.all(np.diff(c, axis=1) > 0) and c.max() < (1 << 20)
    return (np.arange(AUTO_ROWS + 1, dtype=np.int64) * AUTO_ROW_LEN).astype(np.int32), c.ravel().astype(np.int32)


class AutoCase(NamedTuple):
    name: str
    make: Callable
    cols: int
    blocked: bool
    lines: Optional[int]     # distinct lines over the sixteen windows (None: a size gate decides)


AUTO_CASES = [
    AutoCase("at_both_gates", lambda: _auto_scattered(1 << 20, 1 << 22), 1 << 20, True, None),
    AutoCase("cols_one_short", lambda: _auto_scattered((1 << 20) - 1, 1 << 22), (1 << 20) - 1, False, None),
    AutoCase("nnz_one_short", lambda: _auto_scattered(1 << 20, (1 << 22) - 1), 1 << 20, False, None),
    AutoCase("ratio_just_above", lambda: _auto_ratio(+1), 1 << 20, True, 16385),
    AutoCase("ratio_exactly_half", lambda: _auto_ratio(0), 1 << 20, False, 16384),
    AutoCase("ratio_just_below", lambda: _auto_ratio(-1), 1 << 20, False, 16383),
]
AUTO_NAMES = [c.name for c in AUTO_CASES]


@functools.lru_cache(maxsize=None)
def build_auto(name):
    """(rowptr, colids, rows, cols) of an automatic-path case; asserts that the modelled decision and ratio are the intended ones."""
    c = next(a for a in AUTO_CASES if a.name == name)
    rp, ci = c.make()
    nnz = len(ci)
    assert int(rp[-1]) == nnz and ci.min() >= 0 and ci.max() < c.cols
    use, ratio = should_use(AUTO_ROWS, c.cols, nnz, ci)
    assert use == c.blocked, (name, ratio)
    if c.lines is not None:
        assert ratio == c.lines / (PROBE_WINDOW * PROBE_SAMPLES) and (ratio > PROBE_RATIO) == c.blocked
    elif c.blocked:
        assert ratio > 0.9
    for a in (rp, ci):
        a.setflags(write=False)
    return rp, ci, AUTO_ROWS, c.cols
