"""The cases of tests/stream_cases.py are what their names claim, the plan model obeys the properties of a greedy plan (checked without the function
that built it), the union of the cases covers every edge of the row-streaming path (the table EDGES below), and the oracle's fp64 left-to-right sums
— the reference of the bit-identity checks of tests/test_spmv_stream_gpu.py — agree with numpy.longdouble sums. No GPU."""
import numpy as np
import pytest

from tests import stream_cases as sc

TOL = 1e-10                                                             # the project's SpMV bar (tests/test_spmv_gpu.py)
BUILDERS = {"host": sc.host_blocks, "device": sc.device_blocks}


def _lens(m):
    return np.diff(m.rowptr.astype(np.int64))


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_arrays_are_well_formed(name):
    m = sc.build(name)
    assert m.rowptr.dtype == np.int32 and m.colids.dtype == np.int32 and m.values.dtype == np.float64 and m.x.dtype == np.float64
    assert len(m.rowptr) == m.rows + 1 and m.rowptr[0] == 0 and m.rowptr[-1] == len(m.colids) == len(m.values) and len(m.x) == m.cols
    lens = _lens(m)
    assert np.all(lens >= 0) and len(m.colids) <= 150_000 and m.cols >= lens.max(initial=0)
    assert len(m.colids) == 0 or (m.colids.min() >= 0 and m.colids.max() < m.cols)
    ascending = np.ones(len(m.colids), bool)
    ascending[1:] = np.diff(m.colids.astype(np.int64)) > 0
    ascending[m.rowptr[:-1][m.rowptr[:-1] < len(m.colids)]] = True
    assert ascending.all(), "sorted distinct columns in every row"
    assert np.all(np.abs(m.values) <= 1.0) and np.all(np.abs(m.x) <= 1.0)
    # the private columns: referenced once in the whole matrix, by their own row, as its first / last entry
    uses = np.bincount(m.colids, minlength=m.cols)
    for r in np.flatnonzero(lens):
        p = sc.private_cols(m, r)
        assert len(p) == min(2, lens[r]) and all(uses[c] == 1 for c in p)
        assert m.colids[m.rowptr[r]] == p[0] and m.colids[m.rowptr[r + 1] - 1] == p[-1]
    assert np.all(uses[:m.rows][lens == 0] == 0)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", sc.NAMES)
def test_blocks_partition_the_short_rows_and_are_maximal(name, builder):
    m = sc.build(name)
    rp, lens = m.rowptr.astype(np.int64), _lens(m)
    plan = BUILDERS[builder](m.rowptr)
    is_long = lens > sc.TILE_NNZ
    assert plan.long_rows == list(np.flatnonzero(is_long))
    nxt = 0                                                             # the first row no block has taken yet
    for row0, nrows, nnz in plan.blocks:
        while nxt < m.rows and is_long[nxt]:
            nxt += 1
        assert row0 == nxt and nrows >= 1, "in order, no gap, no overlap"
        end = row0 + nrows
        assert not is_long[row0:end].any()
        assert nnz == rp[end] - rp[row0] and nnz <= sc.TILE_NNZ and nrows <= sc.TILE_ROWS
        # maximal: the next row would break a limit, or is long, or there is none, or — device — it lies in the next run
        stops = [end == m.rows, nrows == sc.TILE_ROWS]
        if end < m.rows:
            stops += [bool(is_long[end]), nnz + lens[end] > sc.TILE_NNZ]
            if builder == "device":
                stops.append(end % sc.PLAN_RUN == 0)
        assert any(stops), (row0, nrows, nnz)
        if builder == "device":
            assert row0 // sc.PLAN_RUN == (end - 1) // sc.PLAN_RUN, "no block crosses a run end"
        nxt = end
    while nxt < m.rows and is_long[nxt]:
        nxt += 1
    assert nxt == m.rows
    # the chunks: every long row cut into LONG_CHUNK pieces in entry order, the last one shorter or equal
    want = [(r, k, min(k + sc.LONG_CHUNK, int(rp[r + 1]))) for r in plan.long_rows for k in range(int(rp[r]), int(rp[r + 1]), sc.LONG_CHUNK)]
    assert plan.chunks == want and all(0 < k1 - k0 <= sc.LONG_CHUNK for _, k0, k1 in plan.chunks)
    # the launch: every block is taken by exactly one workgroup of the remapped grid, the others return
    pad, per, grid = sc.launch_geometry(plan)
    taken = [sc.remap(b, plan) for b in range(grid - pad)]
    assert sorted(t for t in taken if t is not None) == list(range(len(plan.blocks)))
    assert pad % sc.XCDS == 0 and 0 <= pad - len(plan.chunks) < sc.XCDS


def test_the_device_plan_is_the_host_plan_of_each_run():
    for name in sc.NAMES:
        m = sc.build(name)
        rp = m.rowptr.astype(np.int64)
        blocks = []
        for a in range(0, m.rows, sc.PLAN_RUN):
            b = min(m.rows, a + sc.PLAN_RUN)
            blocks += [(a + r0, n, nnz) for r0, n, nnz in sc.host_blocks(rp[a:b + 1] - rp[a]).blocks]
        d, h = sc.device_blocks(m.rowptr), sc.host_blocks(m.rowptr)
        assert d.blocks == blocks and d.long_rows == h.long_rows and d.chunks == h.chunks
        assert len(d.blocks) >= len(h.blocks)


def test_lanes_per_row_table():
    """The table DESIGN.md §4.1 (a) records; 127 is the largest row count of a block that takes the shuffle branch."""
    documented = {64: (1, 4), 32: (5, 8), 16: (9, 16), 8: (17, 32), 4: (33, 64), 2: (65, 127)}
    can_group = [n for n in range(1, sc.TILE_ROWS + 1) if n * 2 <= sc.WG and sc.SHORT_ROWS_FACTOR * n < sc.TILE_NNZ]
    assert can_group == list(range(1, 128))
    table = {}
    for n in can_group:
        lo, hi = table.get(sc.tpr_of(n), (n, n))
        table[sc.tpr_of(n)] = (min(lo, n), max(hi, n))
    assert table == documented
    assert sorted(n for pair in documented.values() for n in pair) == sorted(sc.TPR_NROWS)
    assert sc.HEAVY_CAP == 32 and (sc.HEAVY_CAP - 1) * (sc.LANE_ROW_MAX + 1) <= sc.TILE_NNZ < (sc.HEAVY_CAP + 1) * (sc.LANE_ROW_MAX + 1)


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_reaches_the_edge_its_name_claims(name):
    c, m = sc.case(name), sc.build(name)
    cl, lens = c.claims, _lens(m)
    h, d = sc.host_blocks(m.rowptr), sc.device_blocks(m.rowptr)
    if "one_block" in cl:
        assert h.blocks == d.blocks == [(0, m.rows, len(m.colids))] and not h.long_rows
        kind, heavy = sc.reduction_of(h.blocks[0], m.rowptr)
        assert kind == cl["one_block"] and len(heavy) == cl.get("heavy", 0)
        if m.rows >= 4 and name != "rows_128_full":
            assert (lens == 0).any() and (lens == 1).any(), "an empty row and a row of one entry"
        if isinstance(kind, tuple):
            assert len(m.colids) > sc.SHORT_ROWS_FACTOR * m.rows and m.rows * 2 <= sc.WG
        elif kind == "lane":
            assert lens.max() <= sc.LANE_ROW_MAX
    for key, got in (("nrows", m.rows), ("nnz", len(m.colids)), ("chunks", len(h.chunks)), ("n_stream", len(h.blocks)),
                     ("host", len(h.blocks)), ("device", len(d.blocks))):
        if key in cl:
            assert got == cl[key], key
    if "min_rows" in cl:
        assert m.rows >= cl["min_rows"] and m.rows * 2 > sc.WG
        assert np.all(lens[lens > sc.LANE_ROW_MAX] == sc.LANE_ROW_MAX + 1), "heavy rows of 65 entries"
    if name == "heavy_64_65":
        i = int(np.flatnonzero(lens == 65)[0])
        assert lens[i - 1] == 64 and np.sum(lens >= 64) == 2
    if name == "heavy_few_rows":
        assert m.rows * 2 <= sc.WG and len(m.colids) <= sc.SHORT_ROWS_FACTOR * m.rows and lens.max() == 1500
    if "tail" in cl:
        assert len(h.long_rows) == 1 and lens[h.long_rows[0]] == sc.LONG_CHUNK + cl["tail"]
        assert [k1 - k0 for _, k0, k1 in h.chunks] == [sc.LONG_CHUNK, cl["tail"]] and len(h.blocks) >= 2
    if name == "only_long_rows":
        assert np.all(lens > sc.TILE_NNZ) and not h.blocks and not d.blocks
    if cl.get("no_empty_row"):
        assert lens.min() >= 1
        assert sorted({n for _, n, _ in h.blocks}) in ([sc.TILE_ROWS], [1, sc.TILE_ROWS])
    if "len_at" in cl:
        r, n = cl["len_at"]
        assert lens[r] == n and r in (sc.PLAN_RUN - 1, sc.PLAN_RUN) and m.rows > sc.PLAN_RUN + 1
        assert (r in h.long_rows) == (n > sc.TILE_NNZ)
        if n == sc.TILE_NNZ:
            assert (r, 1, n) in h.blocks and (r, 1, n) in d.blocks           # a block of its own in both plans
    if cl.get("cap_at_run_end"):
        assert any(n == sc.TILE_ROWS and (r0 + n) % sc.PLAN_RUN == 0 for r0, n, _ in d.blocks)
    if "empty_run" in cl:
        a = cl["empty_run"] * sc.PLAN_RUN
        assert np.all(lens[a:a + sc.PLAN_RUN] == 0) and lens[a - 1] > 0 and m.rows == 2 * sc.PLAN_RUN + 3
    if name == "run_4096_ones":
        assert m.rows == sc.PLAN_RUN
    if name == "run_4097_ones":
        assert m.rows == sc.PLAN_RUN + 1 and d.blocks[-1] == (sc.PLAN_RUN, 1, 1)
    if name == "empty_everything":
        assert m.rows == 2050 and all(nnz == 0 for _, _, nnz in h.blocks)


# ---- the coverage table: edge → what a case must contain to reach it. H / D: the host / device plan, m: the matrix
def _blocks_with(m, plan, pred):
    return [b for b in plan.blocks if pred(b, *sc.reduction_of(b, m.rowptr))]


def _group_edge(tpr, nrows):
    return lambda m, H, D: _blocks_with(m, H, lambda b, kind, heavy: kind == ("group", tpr) and b[1] == nrows)


def _heavy_edge(count, many_rows):
    return lambda m, H, D: _blocks_with(m, H, lambda b, kind, heavy: len(heavy) == count and (b[1] * 2 > sc.WG) == many_rows)


def _tail_edge(L, loops):
    def reach(m, H, D):
        assert sc.chunk_loops(L)[0] == loops, (L, sc.chunk_loops(L)[0])
        return [c for c in H.chunks if c[2] - c[1] == L]
    return reach


def _len_at(row, n):
    return lambda m, H, D: m.rows > row and _lens(m)[row] == n


EDGES = {}
for _tpr, (_lo, _hi) in {64: (1, 4), 32: (5, 8), 16: (9, 16), 8: (17, 32), 4: (33, 64), 2: (65, 127)}.items():
    EDGES[f"{_tpr} lanes per row, fewest rows ({_lo})"] = _group_edge(_tpr, _lo)
    EDGES[f"{_tpr} lanes per row, most rows ({_hi})"] = _group_edge(_tpr, _hi)
for _n in sc.SWITCH_NROWS:
    EDGES[f"nnzb == 16*nrows, {_n} rows: one lane per row"] = lambda m, H, D, n=_n: _blocks_with(m, H, lambda b, kind, heavy: b[1] == n and b[2] == 16 * n and kind == "lane")
    EDGES[f"nnzb == 16*nrows + 1, {_n} rows: lanes share rows"] = lambda m, H, D, n=_n: _blocks_with(m, H, lambda b, kind, heavy: b[1] == n and b[2] == 16 * n + 1 and isinstance(kind, tuple))
EDGES["129 rows: one lane per row by row count"] = lambda m, H, D: _blocks_with(m, H, lambda b, kind, heavy: b[1] == 129 and b[2] > 0 and kind == "lane")
EDGES["128 rows of 16: nnzb == 16*nrows at TILE_NNZ"] = lambda m, H, D: _blocks_with(m, H, lambda b, kind, heavy: b[1] == 128 and b[2] == sc.TILE_NNZ and kind == "lane")
for _n in sc.HEAVY_COUNTS:
    EDGES[f"{_n} heavy row(s) in one block of > 128 rows"] = _heavy_edge(_n, True)
EDGES["a heavy row in a block of few rows (nnzb <= 16*nrows)"] = _heavy_edge(1, False)
EDGES["a row of 64 entries next to one of 65"] = lambda m, H, D: np.any((_lens(m)[:-1] == sc.LANE_ROW_MAX) & (_lens(m)[1:] == sc.LANE_ROW_MAX + 1)) and \
    _blocks_with(m, H, lambda b, kind, heavy: kind == "lane+heavy")
# chunk length → (trips of the 4×-unrolled loop, trips of the stride-256 tail) of lane 0
for _L, _loops in {1: (0, 1), 255: (0, 1), 256: (0, 1), 257: (0, 2), 769: (1, 0), 1023: (1, 0), 1024: (1, 0), 1025: (1, 1), 2048: (2, 0)}.items():
    EDGES[f"a chunk of {_L} entries"] = _tail_edge(_L, _loops)
for _n, _pad in {2: 6, 8: 0, 9: 7}.items():
    EDGES[f"{_n} chunks, {_pad} padded workgroups"] = lambda m, H, D, n=_n, pad=_pad: len(H.chunks) == n and sc.launch_geometry(H)[0] - n == pad
EDGES["long rows only: n_stream == 0"] = lambda m, H, D: len(H.blocks) == 0 and len(H.chunks) > 0
for _n in sc.NSTREAM:
    EDGES[f"n_stream == {_n}, no empty row"] = lambda m, H, D, n=_n: len(H.blocks) == n and _lens(m).min() >= 1 and not H.chunks
EDGES["4096 rows: one full run"] = lambda m, H, D: m.rows == sc.PLAN_RUN
EDGES["4097 rows: a run of one row"] = lambda m, H, D: m.rows == sc.PLAN_RUN + 1
for _what, _row in (("last row of run 0", sc.PLAN_RUN - 1), ("first row of run 1", sc.PLAN_RUN)):
    EDGES[f"{sc.TILE_NNZ} entries in the {_what}"] = _len_at(_row, sc.TILE_NNZ)
    EDGES[f"{sc.TILE_NNZ + 1} entries in the {_what}"] = _len_at(_row, sc.TILE_NNZ + 1)
EDGES["a run of empty rows only"] = lambda m, H, D: m.rows >= 2 * sc.PLAN_RUN and len(m.colids) > 0 and np.all(_lens(m)[sc.PLAN_RUN:2 * sc.PLAN_RUN] == 0)
EDGES["the row cap reached exactly at a run end"] = lambda m, H, D: [b for b in D.blocks if b[1] == sc.TILE_ROWS and (b[0] + b[1]) % sc.PLAN_RUN == 0]
EDGES["more than one run, host and device block counts equal"] = lambda m, H, D: m.rows > sc.PLAN_RUN and len(H.blocks) == len(D.blocks)
EDGES["a forced cut adds a block"] = lambda m, H, D: len(D.blocks) > len(H.blocks)
EDGES["a forced cut leaves a short one-lane block"] = lambda m, H, D: [b for b in set(D.blocks) - set(H.blocks) if b[1] * 2 <= sc.WG and sc.reduction_of(b, m.rowptr)[0] == "lane"]
EDGES["blocks without an entry"] = lambda m, H, D: len(H.blocks) > 1 and all(b[2] == 0 for b in H.blocks)


def test_the_cases_cover_every_edge():
    plans = {n: (sc.build(n), sc.host_blocks(sc.build(n).rowptr), sc.device_blocks(sc.build(n).rowptr)) for n in sc.NAMES}
    table = {edge: [n for n, (m, H, D) in plans.items() if bool(reach(m, H, D))] for edge, reach in EDGES.items()}
    print("\n".join(f"{edge:62s} {', '.join(names) or '— NONE —'}" for edge, names in table.items()))
    missing = [edge for edge, names in table.items() if not names]
    assert not missing, f"no case reaches: {missing}"
    unused = [n for n in sc.NAMES if not any(n in names for names in table.values())]
    assert all(n.endswith("_full") or n.startswith("run_") for n in unused), f"cases that reach no edge of the table: {unused}"
    assert set(sc.SPMM_NAMES) <= set(sc.NAMES) and len(sc.SEMIRING_NAMES) == 2 * len(sc.TPR_NROWS) + 2 * len(sc.SWITCH_NROWS) + 6 + len(sc.CHUNK_TAILS) + 1


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_equals_longdouble_rows(oracle, name):
    """oracle.spmv (fp64, left to right) is the reference of the bit-identity checks: it agrees with extended-precision sums within the project's bar."""
    m = sc.build(name)
    got = oracle.spmv(m.rowptr, m.colids, m.values, m.x)
    row = np.repeat(np.arange(m.rows, dtype=np.int64), _lens(m))
    terms = m.values.astype(np.longdouble) * m.x[m.colids].astype(np.longdouble)
    want, asum = np.zeros(m.rows, np.longdouble), np.zeros(m.rows, np.longdouble)
    np.add.at(want, row, terms)
    np.add.at(asum, row, np.abs(terms))
    err = np.abs(got.astype(np.longdouble) - want)
    assert np.all(err <= TOL * asum + 1e-300), f"max err / sum|terms| {float(np.max(err / np.maximum(asum, 1e-300)))}"
    assert np.all(got[_lens(m) == 0] == 0.0)
    # and with the plain left-to-right fp64 sum in numpy, bit for bit
    prod = m.values * m.x[m.colids]
    plain = np.array([np.add.accumulate(np.concatenate([[0.0], prod[m.rowptr[r]:m.rowptr[r + 1]]]))[-1] for r in range(m.rows)])
    assert np.array_equal(got, plain)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", sc.NAMES)
def test_emulated_kernel_order_agrees_with_the_oracle(oracle, name, builder):
    """stream_cases.emulate_spmv restates the kernels' additions in their order (what the GPU test demands bit for bit of EVERY row): its one-lane rows
    are the oracle's bits, every row is within the project's bar of the oracle, and the rows several lanes share do take another order somewhere."""
    m = sc.build(name)
    plan = BUILDERS[builder](m.rowptr)
    got, want = sc.emulate_spmv(m, plan), oracle.spmv(m.rowptr, m.colids, m.values, m.x)
    _, asum = oracle.spmv_ld(m.rowptr, m.colids, m.values, m.x)
    assert np.all(np.abs(got - want) <= TOL * asum + 1e-300)
    lane = sc.row_kinds(m.rowptr, plan) == "lane"
    assert np.array_equal(got[lane], want[lane])
