"""The cases of tests/pb_cases.py reach the edges of the blocked SpMV path they are named for — asserted on the numbers of the numpy model of
pb_build: item lengths, hot bands, empty bands, slots of the degree hash — at both band widths, and their union covers every edge the GPU test
(tests/test_spmv_pb_limits_gpu.py) is meant to pin. The modelled layout is a valid plan: the product computed through it (pb_cases.emulate) equals a
long-double row-by-row product for every case under the environment the GPU test gives it. The model's constants are the source's. No GPU."""
import os
import re

import numpy as np
import pytest

from tests import pb_cases as pc
from tests import structured_cases as sc

WIDTHS = (pc.BAND_NARROW, pc.BAND_WIDE)
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "g4s_amd", "csrc", "spmv_pb.hip")
ALPHA_BETA = ((1.0, 0.0), (-2.5, 0.75))
both = pytest.mark.parametrize("W", WIDTHS)


def _item_entries(P):
    return [(s1 - s0) * pc.SPAN for _, s0, s1 in P.pitems]


def _band_items(P, c):
    return sorted((s0, s1) for cb, s0, s1 in P.pitems if cb == c)


@both
@pytest.mark.parametrize("name", pc.NAMES)
def test_case_reaches_its_edge(name, W):
    c, m, P = pc.case(name), pc.build(name, W), pc.model(name, W)
    cl = c.claims
    assert m.rowptr.dtype == np.int32 and m.colids.dtype == np.int32 and m.rowptr[0] == 0 and m.rowptr[-1] == len(m.colids) == P.nnz
    assert len(m.colids) < pc.PB_MIN_NNZ // 8, "as small as the edge allows"
    assert not (m.cols >= pc.BIN_MIN_COLS and P.nnz >= pc.BIN_MIN_NNZ), "the hashed degree count, not the binned one"
    deg = np.bincount(m.colids, minlength=m.cols)
    if "shape" in cl:
        assert (m.rows, m.cols) == cl["shape"]
    if "bands" in cl:
        assert (P.CB, P.RB) == cl["bands"]
    if cl.get("below_band"):
        assert 1 < m.rows < pc.BAND_NARROW and 1 < m.cols < pc.BAND_NARROW
    if cl.get("every_column"):
        assert m.rows == 1 and np.all(deg == 1) and P.CB >= 3
    if cl.get("every_row"):
        assert m.cols == 1 and np.all(np.diff(m.rowptr) == 1) and P.RB >= 3
    for key in ("Hmax", "H"):
        if key in cl:
            assert getattr(P, key) == cl[key], key
    if name.startswith("cols_2w_minus_1"):
        assert m.cols == 2 * W - 1
    elif name.startswith("cols_2w"):
        assert m.cols == 2 * W
    if cl.get("ranked"):
        assert c.hot is None and len(P.in_band) >= 1                 # the ranking ran and the automatic rule looked at a band
    if cl.get("clamped"):
        assert c.hot > P.Hmax == P.H > 0
    if "empty_row_bands" in cl:
        empty = cl["empty_row_bands"]
        assert empty[-1] == P.RB - 1 and 0 < empty[0] < P.RB - 1     # the last band and one in the middle
        for r in empty:
            assert r * W < m.rows and P.band_start[r] == P.band_end[r] == P.band_start[r + 1]
            assert [it for it in P.citems if it[0] == r] == [(r, int(P.band_start[r]), int(P.band_start[r]), 0)]   # k1 == k0: its rows must still be written
        assert all(P.band_end[r] > P.band_start[r] for r in range(P.RB) if r not in empty)
    if "split" in cl:
        assert P.split == cl["split"]
    if "empty_col_bands" in cl:
        empty = cl["empty_col_bands"]
        assert empty[-1] == P.CBnat - 1 and 0 < empty[0] < P.CBnat - 1
        for b in range(P.CBnat):
            assert (len(_band_items(P, P.H + b)) == 0) == (b in empty)
    if "exact_band" in cl:
        b = cl["exact_band"]
        assert P.in_band[b] * P.CBnat == int(pc.HOT_FACTOR) * P.nnz                 # exactly kHotFactor · nnz / CBnat, in integers …
        assert float(P.in_band[b]) == pc.HOT_FACTOR * (float(P.nnz) / P.CBnat)     # … and in the doubles the comparison is made in
        assert P.H == b + 1 < P.Hmax and P.in_band[b + 1] < P.in_band[b]
    if "short_by" in cl:
        assert P.in_band[0] * P.CBnat == int(pc.HOT_FACTOR) * P.nnz - cl["short_by"] * P.CBnat and P.H == 0
    if "exact_band" in cl or "short_by" in cl:
        # a degree one short (exact) or one over (short) on a column of the deciding band changes H: the device's count must be exact
        b = cl.get("exact_band", 0)
        _, order = pc.rank_columns(m.colids, m.cols)
        for col in (order[b * W], order[b * W + pc.HASH_POPULAR // 2]):
            off = deg.copy()
            off[col] += -1 if "exact_band" in cl else 1
            Q = pc.plan(m.rowptr, m.colids, m.rows, m.cols, W, hot=c.hot, deg=off)
            assert Q.H != P.H and Q.debug_fields() != P.debug_fields()
    if cl.get("tie"):
        ranked_deg, order = pc.rank_columns(m.colids, m.cols)
        edge = P.H * W
        assert ranked_deg[order[edge - 1]] == ranked_deg[order[edge]] > ranked_deg[order[edge + pc.TIE_EXTRA]]
        assert np.all(np.diff(order[edge - W:edge + pc.TIE_EXTRA]) > 0)         # the tied columns in ascending id order: the lowest W are hot
        Q = pc.plan(m.rowptr, m.colids, m.rows, m.cols, W, hot=c.hot, ties="descending")
        assert set(Q.hot_cols.tolist()) != set(P.hot_cols.tolist())
        assert (Q.padded, Q.micro_runs) != (P.padded, P.micro_runs), "the debug line would not notice the other tie order"
    if cl.get("hash_collisions"):
        pop = pc.hash_popular_columns(W)
        assert len(np.unique(pc.deg_hash(pop))) <= pc.HASH_SLOTS and np.all(deg[pop] >= pc.HASH_DEGREE - 1)
        assert set(pop.tolist()) <= set(P.hot_cols.tolist()) or P.H == 0
        slot_of = dict(zip(pop.tolist(), pc.deg_hash(pop).tolist()))
        contested = 0
        for k0, k1 in pc.deg_block_shares(P.nnz):
            share = np.unique(m.colids[k0:k1])
            slots = [slot_of[col] for col in share.tolist() if col in slot_of]
            per_slot = np.bincount(np.array(slots, np.int64), minlength=1)
            contested += int(np.sum(per_slot >= 2))                              # one column owns the slot in LDS, the others go to HBM
        assert contested >= 200
    if "items" in cl:
        assert sorted(_item_entries(P)) == sorted(cl["items"])
        assert P.kPC * pc.SPAN == max(pc.PCHUNK_FLOOR, c.pchunk) // pc.WINDOW * pc.WINDOW
        if c.pchunk < pc.PCHUNK_FLOOR:
            assert P.kPC * pc.SPAN == pc.PRODUCER_STEP                          # the floor: items of exactly one STEP
    if cl.get("last_window"):
        tails = [_band_items(P, b)[-1] for b in range(P.CB) if len(_band_items(P, b)) > 1]
        assert any((s1 - s0) * pc.SPAN == pc.WINDOW for s0, s1 in tails)
        s0, s1 = next(t for t in tails if (t[1] - t[0]) * pc.SPAN == pc.WINDOW)
        live = int(np.sum(P.p_row[s0 * pc.SPAN:s1 * pc.SPAN] >= 0))
        assert 0 < live < pc.WINDOW                                             # with pads in its tail
    if "hub_row" in cl:
        hub = cl["hub_row"]
        at = np.flatnonzero((P.p_row == hub) & (P.p_band == 0))
        assert len(at) == W and np.all(np.diff(at) == 1)
        cuts = [s0 * pc.SPAN for s0, _ in _band_items(P, 0)[1:]]
        assert len(cuts) >= 2 and all(at[0] < cut <= at[-1] for cut in cuts)
        assert at[0] > 0 and P.p_row[at[-1] + 1] >= 0                          # entries of other rows before and behind it
    if "item_slots" in cl:
        n = cl["item_slots"]
        assert P.kCC == n == max(pc.CCHUNK_FLOOR, c.cchunk & ~3)
        lens = [k1 - k0 for _, k0, k1, s in P.citems if s]
        assert lens and max(lens) == n
        if "full_items" in cl:
            assert lens.count(n) == cl["full_items"] and sorted(v for v in lens if v != n) == ([cl["tail"]] if cl["tail"] else [])
        else:
            assert lens.count(n) >= 50 and c.cchunk <= 4
    if cl.get("hub_local_row0"):
        item = max(P.citems, key=lambda it: pc.wave_branches(P, it)[0])
        uniform, _ = pc.wave_branches(P, item)
        assert uniform >= 2
        _, k0, k1, _ = item
        assert np.all(P.c_lrow[k0:k0 + 256 * uniform] == 0), "the hub is local row 0, the row the pad slots name"
    if cl.get("tail_wave_on_one_row"):
        assert all(pc.tail_wave_on_one_row(P, it) for it in P.citems)
    if name == "one_row" and W == pc.BAND_NARROW:
        assert pc.tail_wave_on_one_row(P, P.citems[0]) and pc.wave_branches(P, P.citems[0]) == (4, 1)   # four whole waves and a tail wave of one group on the same row
    if "uniform_waves" in cl:
        item = max(P.citems, key=lambda it: pc.wave_branches(P, it)[0])
        _, k0, k1, _ = item
        assert pc.wave_branches(P, item)[0] == cl["uniform_waves"] and pc.wave_branches(P, item)[1] >= 1
        run = int(np.argmax(P.c_lrow[k0:k1] != 0))                              # the hub's run: the first `run` slots of the item
        assert run % 256 != 0 and run // 256 == cl["uniform_waves"], "the run ends inside a wave: that wave takes the per-lane branch"


def test_union_covers_every_edge():
    cl = {c.name: c.claims for c in pc.CASES}
    have = lambda key, value=None: [n for n, d in cl.items() if key in d and (value is None or d[key] == value)]
    assert have("shape", (1, 1)) and have("every_column") and have("every_row") and have("below_band")
    assert {pc.case(n).hot for n in have("Hmax", 0)} == {None, 3} and have("ranked") and [n for n in have("Hmax", 1) if pc.case(n).hot is None]
    assert have("empty_row_bands") and have("split") and have("empty_col_bands")
    assert have("exact_band", 0) and have("short_by", 1) and have("exact_band", 1) and have("tie") and len(have("clamped")) >= 2
    assert len(have("hash_collisions")) == 2
    items = [v for n in have("items") for v in cl[n]["items"]]
    S = pc.PRODUCER_STEP
    assert {S, 2 * S + pc.WINDOW, pc.WINDOW} <= set(items) and have("last_window") and have("hub_row")
    assert any(pc.case(n).pchunk < pc.PCHUNK_FLOOR for n in have("items"))
    C = pc.CONSUMER_STEP
    assert {cl[n]["item_slots"] for n in have("item_slots")} == {4, C, C + 4, 2 * C + 4}
    assert any(pc.case(n).cchunk < pc.CCHUNK_FLOOR for n in have("item_slots")) and have("uniform_waves") and len(have("hub_local_row0")) >= 2
    assert have("tail_wave_on_one_row")
    assert {pc.case(n).group for n in pc.UPDATABLE_NAMES} == set(pc.GROUPS)
    # unsplit and split bands, hot and cold bands all occur (the NaN-in-y and NaN-in-x checks of the GPU test need them)
    plans = [pc.model(n, W) for n in pc.NAMES for W in WIDTHS]
    assert any(P.split for P in plans) and any(len(P.split) < P.RB for P in plans) and any(P.H for P in plans) and any(P.H == 0 for P in plans)


def _longdouble_product(m, values, x, alpha, beta, y0):
    terms = values.astype(np.longdouble) * x[m.colids].astype(np.longdouble)
    want, asum = np.zeros(m.rows, np.longdouble), np.zeros(m.rows, np.longdouble)
    row = pc.row_of(m.rowptr)
    np.add.at(want, row, terms)
    np.add.at(asum, row, np.abs(terms))
    return np.longdouble(alpha) * want + (np.longdouble(beta) * y0 if beta != 0.0 else 0.0), asum


@both
@pytest.mark.parametrize("name", pc.NAMES)
def test_emulated_layout_gives_the_product(name, W):
    m, P = pc.build(name, W), pc.model(name, W)
    for alpha, beta in ALPHA_BETA:
        got = pc.emulate(P, m.values, m.x, alpha, beta, m.y0)
        want, asum = _longdouble_product(m, m.values, m.x, alpha, beta, m.y0)
        assert not np.isnan(got).any(), "a row no item writes"
        assert np.all(np.abs(got - want) <= 1e-17 * (abs(alpha) * asum + abs(beta) * np.abs(m.y0)) + 1e-300)
    for beta in (0.0, 1.0):                                                    # integer data: exact, whatever the order
        got = pc.emulate(P, m.ivalues, m.ix, 1.0, beta, m.iy0)
        want, _ = _longdouble_product(m, m.ivalues, m.ix, 1.0, beta, m.iy0)
        assert np.array_equal(got, want) and np.all(np.abs(want) < 2 ** 53)


@both
@pytest.mark.parametrize("name", pc.NAMES)
def test_layout_invariants(name, W):
    m, P = pc.build(name, W), pc.model(name, W)
    assert P.padded % pc.WINDOW == 0 and np.all(P.cell_start % pc.SPAN == 0) and np.all(P.cell_start[::P.RB][:-1] % pc.WINDOW == 0)
    assert np.array_equal(np.sort(P.pos), np.flatnonzero(P.p_row >= 0)) and np.array_equal(P.p_src[P.pos], np.arange(P.nnz))
    assert np.all(P.p_local[P.p_row < 0] == W) and np.all(P.p_local[P.pos] == P.col_local[m.colids]) and np.all(P.p_band[P.pos] == P.col_band[m.colids])
    assert len(np.unique(P.col_band * (1 << 15) + P.col_local)) == m.cols      # the column map is one to one
    assert P.micro_runs == int(P.head.sum()) == len(np.unique(P.run_slot)) and P.nnz >= P.micro_runs >= 1
    assert np.all(P.band_start % 4 == 0) and np.all(P.band_end <= P.band_start[1:]) and np.all(P.band_start[1:] - P.band_end < 4)
    # heads restated per span, as pb_span_heads_kernel walks them
    t_cell = np.full(P.padded, 0, np.int64)
    t_cell[P.pos] = P.col_band[m.colids] * P.RB + pc.row_of(m.rowptr) // W
    spans = np.random.default_rng(1).choice(P.padded // pc.SPAN, min(400, P.padded // pc.SPAN), replace=False)
    for s in spans.tolist() + [0, P.padded // pc.SPAN - 1]:
        a = s * pc.SPAN
        prev = -2
        if a % pc.WINDOW != 0 and P.p_row[a] >= 0 and P.p_row[a - 1] >= 0 and t_cell[a] == t_cell[a - 1]:
            prev = P.p_row[a - 1]
        for j in range(pc.SPAN):
            r = P.p_row[a + j]
            assert bool(P.head[a + j]) == (r >= 0 and r != prev)
            if r >= 0:
                prev = r


def _source():
    with open(SOURCE) as f:
        return f.read()


def test_constants_are_the_sources():
    src = _source()
    for pattern, value in ((r"constexpr int kBandWide = (\d+);", pc.BAND_WIDE), (r"constexpr int kBandNarrow = (\d+);", pc.BAND_NARROW),
                           (r"constexpr int kSpan = (\d+);", pc.SPAN), (r"constexpr int kWindow = (\d+);", pc.WINDOW),
                           (r"constexpr int kMaxHotBands = (\d+);", pc.MAX_HOT_BANDS), (r"constexpr int kPbThreads = (\d+);", pc.PB_THREADS),
                           (r"#define G4S_PB_PAIR_UNROLL (\d+)", pc.PAIR_UNROLL), (r"#define G4S_PB_CONS_UNROLL (\d+)", pc.CONS_UNROLL),
                           (r"constexpr int kProducerChunk = 1 << (\d+);", 17), (r"constexpr int kConsumerChunk = 1 << (\d+);", 17),
                           (r"constexpr int kDegSlots = (\d+), kDegBlocks = \d+;", pc.DEG_SLOTS), (r"kDegSlots = \d+, kDegBlocks = (\d+);", pc.DEG_BLOCKS),
                           (r"\(unsigned\)c \* (\d+)u\) >> 20", pc.DEG_HASH_MUL), (r"auto_pc = .*std::max<long long>\((\d+), pow2_at_most\(totP / 128\)", pc.AUTO_PC_FLOOR),
                           (r"auto_cc = .*std::max<long long>\((\d+), pow2_at_most\(P->micro_runs / 128\)", pc.AUTO_CC_FLOOR),
                           (r"const int W = (\d+), S = \d+;", pc.PROBE_WINDOW), (r"const int W = \d+, S = (\d+);", pc.PROBE_SAMPLES),
                           (r"h\[i\] >>= (\d+);", pc.PROBE_LINE_SHIFT)):
        found = re.findall(pattern, src)
        assert len(found) == 1 and int(found[0]) == value, pattern
    assert (pc.PRODUCER_CHUNK, pc.CONSUMER_CHUNK) == (1 << 17, 1 << 17)
    assert float(re.search(r"constexpr double kHotFactor = ([\d.]+);", src).group(1)) == pc.HOT_FACTOR
    for line in ("constexpr int STEP = kPbThreads * kPairUnroll;", "constexpr int STEP = 4 * kPbThreads * kPbUnroll;",
                 "const int Hmax = std::min(kMaxHotBands, cols / (2 * W));", "if ((double)in_band < kHotFactor * avg) break;",
                 "std::max<long long>(kSpan * kPbThreads, getenv(\"G4S_PB_PCHUNK\")", "std::max<long long>(4, (getenv(\"G4S_PB_CCHUNK\")",
                 "if ((long long)cols * 8 < (8ll << 20) || nnz < (4ll << 20)) return false;", "return ratio / S > 0.5;",
                 "if (cols >= (1 << 20) && nnz >= (1ll << 24)"):
        assert line in src, line
    assert pc.PRODUCER_STEP == 8192 and pc.CONSUMER_STEP == 8192


def test_size_gates_are_shared_with_the_structured_model():
    assert sc.PB_MIN_X_BYTES is pc.PB_MIN_X_BYTES and sc.PB_MIN_NNZ is pc.PB_MIN_NNZ
    assert (pc.PB_MIN_X_BYTES, pc.PB_MIN_NNZ) == (8 << 20, 4 << 20)
    ci = np.zeros(8, np.int32)
    assert pc.should_use(10, (pc.PB_MIN_X_BYTES // 8) - 1, 1 << 30, ci) == (False, None)
    assert pc.should_use(10, 1 << 30, pc.PB_MIN_NNZ - 1, ci) == (False, None)


@pytest.mark.parametrize("name", pc.AUTO_NAMES)
def test_automatic_path_cases_sit_on_their_side(name):
    c = next(a for a in pc.AUTO_CASES if a.name == name)
    rp, ci, rows, cols = pc.build_auto(name)                                    # asserts the decision and the exact ratio
    nnz = len(ci)
    use, ratio = pc.should_use(rows, cols, nnz, ci)
    assert use == c.blocked and rows == len(rp) - 1
    assert abs(cols - (1 << 20)) <= 1 and abs(nnz - (1 << 22)) <= 1
    assert (cols * 8 >= pc.PB_MIN_X_BYTES and nnz >= pc.PB_MIN_NNZ) == (ratio is not None)
    if c.lines is not None:
        stride = (nnz - pc.PROBE_WINDOW) // pc.PROBE_SAMPLES
        lines = sum(len(np.unique(ci[w * stride:w * stride + pc.PROBE_WINDOW] >> 4)) for w in range(pc.PROBE_SAMPLES))
        assert lines == c.lines and abs(lines - 16384) <= 1
    # the structured model defers to the probe: the path of a handle created without a path flag
    assert sc.expected_path(rows, cols, rp, ci) == (pc.PATH_BLOCKED if c.blocked else sc.PATH_STREAM)
    assert sc.expected_path(rows, cols, rp, ci, force_stream=True) == sc.PATH_STREAM
