"""The cases of tests/masked_cases.py are what their names claim: every row has exactly the mask length, the entries of A and the products its descriptor
declares (counted here from the index arrays, not by the builders), the classes written by hand at the builders are the model's, the "at" and "just past" rows
of every pair differ by that cut alone, every edge of COVERAGE is stood on by a named row with the declared numbers in a mode that the GPU test runs, the model
notices each of its six numbers moving by one, and the reference gives hits and identities where a row is meant to show both. No GPU."""
import functools

import numpy as np
import pytest

from tests import masked_cases as mc
from tests import masked_ref


@functools.lru_cache(maxsize=None)
def _ref(name, semiring, pattern_only=False):
    c = mc.build(name)
    A, B = mc.operands(c, semiring)
    out = masked_ref.spgemm_masked(A, B, c.M, c.N, c.mask, semiring, pattern_only)
    for a in out:
        a.setflags(write=False)
    return out


def _counts(c):
    arp, aci, _ = c.A
    blen = np.diff(c.B[0].astype(np.int64))
    na = np.diff(arp).astype(np.int64)
    flop = np.zeros(c.M, np.int64)
    np.add.at(flop, np.repeat(np.arange(c.M), na), blen[aci])
    return np.diff(c.mask[0]).astype(np.int64), na, flop


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_is_well_formed_and_every_row_has_its_declared_counts(name):
    c = mc.build(name)
    (arp, aci, ava), (brp, bci, bva), (mrp, mci) = c.A, c.B, c.mask
    assert arp.dtype == brp.dtype == aci.dtype == bci.dtype == mrp.dtype == mci.dtype == np.int32 and ava.dtype == bva.dtype == np.float64
    assert len(arp) == len(mrp) == c.M + 1 and len(brp) == c.K + 1 and arp[0] == brp[0] == mrp[0] == 0
    assert arp[-1] == len(aci) == len(ava) and brp[-1] == len(bci) == len(bva) and mrp[-1] == len(mci) > 0
    assert len(c.rows) == c.M and c.semirings == mc.semirings_of(name)
    for rp, ci, width in ((arp, aci, c.K), (brp, bci, c.N), (mrp, mci, c.N)):
        assert np.all(np.diff(rp) >= 0) and (len(ci) == 0 or (ci.min() >= 0 and ci.max() < width)), "all ids in range"
    for rp, ci in ((brp, bci), (mrp, mci)):                            # (A's rows are in the order the tiles ask for, B's and the mask's ascend)
        up = np.ones(len(ci), bool)
        up[1:] = np.diff(ci.astype(np.int64)) > 0
        up[rp[:-1][rp[:-1] < len(ci)]] = True
        assert up.all(), "strictly ascending rows"
    for v in (ava, bva):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 4
    assert (bva == 0).any() or bva.size < 40, "exact zeros are kept"
    mlen, na, flop = _counts(c)
    for i, r in enumerate(c.rows):
        assert (r.mlen, r.na, r.flop) == (mlen[i], na[i], flop[i]), (r.tag, mlen[i], na[i], flop[i])
    assert 0 < flop.sum() <= 2_200_000, "the reference multiplies a case in seconds"
    for r in c.rows:                                                   # the classes written by hand are the model's
        assert dict(r.cls).keys() == set(mc.RUNS[name])
        for mode, cls in r.declared:
            assert mode in mc.RUNS[name] and mc.cls_of(r, mode) == cls, (r.tag, mode, cls, mc.cls_of(r, mode))


def test_class_rule_at_every_cut_and_the_clamps():
    d = mc.cuts_of({})
    assert d == {"wave_mask": 64, "wave_flop": 4096, "split_flop": 1 << 20, "lds_small": 1024, "lds_large": 8192, "split_ways": 128}
    cls = lambda m, f, cuts=d: mc.row_class(m, f, cuts)
    assert [cls(m, f) for m in (1, 63, 64, 65) for f in (1, 4095, 4096, 4097)] == ["wave"] * 3 + ["lds_small"] + ["wave"] * 3 + ["lds_small"] + ["wave"] * 3 + ["lds_small"] * 5
    assert (cls(1024, 5000), cls(1025, 5000), cls(8192, 5000), cls(8193, 5000)) == ("lds_small", "lds_large", "lds_large", "global")
    assert (cls(1024, 1 << 20), cls(1024, (1 << 20) + 1), cls(1025, 1 << 20), cls(1025, (1 << 20) + 1)) == ("lds_small", "split_lds", "lds_large", "split_global")
    assert (cls(1, (1 << 20) + 1), cls(8193, (1 << 20) + 1), cls(8193, 1)) == ("split_lds", "split_global", "global")
    assert cls(0, 5) == cls(5, 0) == cls(0, 0) == cls(0, 1 << 30) == "skip"
    env = lambda **kw: mc.cuts_of({f"G4S_MASKED_{k}": str(v) for k, v in kw.items()})
    assert env(LDS_SMALL=4000)["lds_small"] == 1024 and env(LDS_LARGE=100000)["lds_large"] == 8192, "only downwards"
    assert env(LDS_SMALL=-5)["lds_small"] == 0 and env(LDS_LARGE=0)["lds_large"] == 0
    assert env(SPLIT_WAYS=1)["split_ways"] == 2 and env(SPLIT_WAYS=5000)["split_ways"] == 4096 and env(SPLIT_FLOP=0)["split_flop"] == 1
    assert env(WAVE_FLOP=-1)["wave_flop"] == 0 and env(WAVE_FLOP=1 << 40)["wave_flop"] == 1 << 30
    assert mc.cuts_of({"G4S_MASKED_LDS_SMALL": ""}) == d, "an empty variable is no variable"
    assert cls(10, 50, env(WAVE_FLOP=0)) == "lds_small" and cls(10, 50, env(LDS_SMALL=0)) == "wave" and cls(70, 50, env(LDS_SMALL=0)) == "lds_large"
    assert cls(70, 50, env(LDS_SMALL=0, LDS_LARGE=0)) == "global" and cls(70, 50, env(LDS_LARGE=0)) == "lds_small", "the small table is asked first"
    assert cls(70, 20001, env(SPLIT_FLOP=20000, LDS_SMALL=0)) == "split_global"
    assert mc.cuts_of(mc.MODES["lds_over"]) == d


@pytest.mark.parametrize("name", mc.NAMES)
def test_at_and_past_rows_differ_by_that_cut_alone(name):
    c = mc.build(name)
    for e in c.edges:
        assert e.mode in mc.RUNS[name] and e.at_cls != e.past_cls, e
        at, past = mc.row(c, e.at), mc.row(c, e.past)
        assert (mc.cls_of(at, e.mode), mc.cls_of(past, e.mode)) == (e.at_cls, e.past_cls), e
        cuts = mc.cuts_of(mc.MODES[e.mode])
        on = {"wave_mask": (at.mlen, past.mlen), "wave_flop": (at.flop, past.flop), "split_flop": (at.flop, past.flop), "lds_small": (at.mlen, past.mlen),
              "lds_large": (at.mlen, past.mlen)}[e.const]
        assert on == (cuts[e.const], cuts[e.const] + 1), e
        assert mc.row_class(past.mlen, past.flop, {**cuts, e.const: cuts[e.const] + 1}) == e.at_cls, f"{e}: with the cut one higher the past row joins the other"
        assert mc.row_class(at.mlen, at.flop, {**cuts, e.const: cuts[e.const] - 1}) == e.past_cls, f"{e}: with the cut one lower the at row joins the other"


WANTED = (["grid_m%d_f%d" % (m, f) for m in (1, 63, 64, 65) for f in (1, 4095, 4096, 4097)]
          + ["mlen_1024_with_1025", "mlen_8192_with_8193", "flop_2p20_small_mask", "flop_2p20_mlen_1025", "split_row_mlen_1024_with_1025", "skip_mask_without_products",
             "skip_products_without_mask", "env_wave_flop_100", "env_lds_small_100", "env_lds_large_2000", "env_split_flop_20000", "env_split_ways_2", "env_split_ways_3",
             "env_lds_small_0", "env_lds_large_0", "env_clamp_above_range"]
          + ["wave_na_%d" % n for n in (1, 63, 64, 65, 128, 129)]
          + ["wave_empty_b_rows_in_tile", "wave_tile_all_empty", "wave_tile_total_64_65_128", "wave_below_every_mask_column", "wave_above_every_mask_column",
             "wave_first_and_last_mask_column", "wave_column_n_minus_1"] + ["wave_rows_%d" % n for n in (1, 3, 4, 5)]
          + ["row256_na_%d" % n for n in (255, 256, 257, 512, 513)] + ["row256_clip", "row256_mlen_1", "row256_table_full"]
          + ["row1024_na_%d" % n for n in (1023, 1024, 1025, 2049)] + ["row1024_table_full", "row1024_every_slot", "global_mlen_8193", "global_full_width"]
          + ["split_tiles_fewer_than_ways", "split_ways_second_round", "split_sums_to_zero", "split_slots_without_products", "split_three_rows_or_more"]
          + ["only_wave", "only_lds_small", "only_lds_large", "only_global", "only_split_lds", "only_split_global", "all_seven_classes", "only_wave_and_global"]
          + ["open_%d" % M for M in (1, 31, 32, 33)])


def test_every_edge_is_covered_by_a_named_row_in_a_mode_that_runs():
    assert set(WANTED) == set(mc.COVERAGE)
    for edge, entries in mc.COVERAGE.items():
        assert entries, edge
        for name, tag, mode, want in entries:
            assert mode in mc.RUNS[name] and mode in mc.MODES, (edge, name, mode)
            r = mc.row(mc.build(name), tag)                            # StopIteration: no such row
            for field, value in want.items():
                got = mc.cls_of(r, mode) if field == "cls" else getattr(r, field)
                assert got == value, (edge, name, tag, mode, field, got, value)
    assert set(mc.RUNS) == set(mc.NAMES) and all("default" in m for m in mc.RUNS.values())
    assert {m for modes in mc.RUNS.values() for m in modes} == set(mc.MODES), "a mode that no case runs"
    assert set(mc.HOST_FORM) <= set(mc.NAMES)


def _present(name, mode):
    counts = mc.expected_counts(mc.build(name), mode)
    return {k for k in mc.CLASSES if counts[k]}


def test_the_class_lists_the_cases_are_built_for():
    """one class alone besides skip, all seven at once, a gap in the middle; 1, 3, 4 and 5 wave rows; three split rows or more where `blockIdx.x / ways` counts"""
    for n in (1, 3, 4, 5):
        assert _present(f"wave_rows_{n}", "default") == {"skip", "wave"} and mc.expected_counts(mc.build(f"wave_rows_{n}"), "default")["wave"] == n
    assert sorted(n % mc.WAVE_ROWS_PER_WG for n in (1, 3, 4, 5)) == [0, 1, 1, 3], "a last workgroup of one, of three and of four rows, and a second one of one"
    assert {mc.row(mc.build("row1024"), f"na_{na}").na - mc.WG_LARGE for na in (1023, 1024, 1025)} == {-1, 0, 1} and mc.row(mc.build("row1024"), "na_2049").na == 2 * mc.WG_LARGE + 1
    assert mc.OPEN_ROWS_PER_WG == 32
    for cls, (_, mode) in mc._ONLY.items():
        assert _present(f"only_{cls}", mode) == {"skip", cls} and mc.expected_counts(mc.build(f"only_{cls}"), mode)[cls] == 3
    assert _present("moved", "split_flop_20000") == set(mc.CLASSES)
    assert _present("wave_and_global", "default") == {"skip", "wave", "global"}
    for mode in ("split_flop_20000", "split_ways_2", "split_ways_3"):
        counts = mc.expected_counts(mc.build("moved"), mode)
        assert counts["split_lds"] >= 3 and counts["split_global"] >= 2
    # one case per class goes through the host-pointer form
    host = set().union(*(_present(n, m) for n in mc.HOST_FORM for m in mc.RUNS[n]))
    assert host == set(mc.CLASSES)


def test_split_rows_have_the_tiles_their_names_claim():
    c = mc.build("split_mlen_1024")
    r = mc.row(c, "flop_2p20_plus_1")
    tiles = -(-r.na // mc.WG)
    assert r.na % mc.WG == 0 and tiles == 4 < mc.SPLIT_WAYS, "part 4 starts exactly at the row's end, parts 5 … 127 behind it"
    m = mc.build("moved")
    for tag, na in (("flop_20001_na_512_m1024", 512), ("flop_20001_na_513", 513), ("flop_20001_na_768_m1025", 768), ("flop_20001_na_769_m1024", 769)):
        assert mc.row(m, tag).na == na and na in (2 * mc.WG, 2 * mc.WG + 1, 3 * mc.WG, 3 * mc.WG + 1)
    # the rounds of `for (a0 = first; a0 < ae; a0 += ways·TPB)`: with 2 parts 513 entries give part 0 a second round and part 1 none; with 3 parts 769 do
    rounds = lambda na, ways: [len(range(part * mc.WG, na, ways * mc.WG)) for part in range(ways)]
    assert rounds(512, 2) == [1, 1] and rounds(513, 2) == [2, 1] and rounds(768, 2) == [2, 1] and rounds(769, 2) == [2, 2]
    assert rounds(768, 3) == [1, 1, 1] and rounds(769, 3) == [2, 1, 1] and rounds(512, 3) == [1, 1, 0] and rounds(513, 3) == [1, 1, 1]


def test_the_opening_pass_cases():
    for M in (1, 31, 32, 33):
        c = mc.build(f"open_{M}")
        assert c.M == M and {r.mlen for r in c.rows} == {(i + 3) % 10 for i in range(M)}
    mrp, mci = mc.build("open_33").mask
    assert set(np.diff(mrp)) == set(range(10)) and mc.OPEN_LPR in np.diff(mrp), "fewer, as many and more entries than the 8 lanes"
    starts_below = [i for i in range(1, 33) if mrp[i + 1] > mrp[i] and mrp[i] > mrp[i - 1] and mci[mrp[i]] < mci[mrp[i] - 1]]
    assert len(starts_below) >= 5, "rows that start below the last column of the row before them: valid, and must be accepted"
    for name in mc.NAMES:                                              # products = Σ flop over the rows with a mask row and products
        c = mc.build(name)
        mlen, _, flop = _counts(c)
        for mode in mc.RUNS[name]:
            assert mc.expected_counts(c, mode)["products"] == int(flop[(mlen > 0) & (flop > 0)].sum())
            assert sum(mc.expected_counts(c, mode)[k] for k in mc.CLASSES) == c.M
            assert sum(mc.expected_info(c, mode).values()) >= c.M - mc.expected_counts(c, mode)["skip"]


@pytest.mark.parametrize("const", ["wave_mask", "wave_flop", "lds_small", "lds_large", "split_flop"])
@pytest.mark.parametrize("step", [-1, 1])
def test_model_notices_each_default_number_moving_by_one(const, step):
    """On the model only: with one of the default numbers one lower or one higher, the expected counts of some case in the DEFAULT environment change — a library
    built with that number off by one could not print the lines the GPU test asks for. (split_ways moves no row to another class; its cases compare values.)"""
    base = mc.cuts_of({})
    moved = {**base, const: base[const] + step}
    changed = [n for n in mc.NAMES if mc.expected_counts(mc.build(n), "default", moved) != mc.expected_counts(mc.build(n), "default")]
    assert changed, f"{const} {step:+d} goes unnoticed"


@pytest.mark.parametrize("mode,const", [("wave_flop_100", "wave_flop"), ("lds_small_100", "lds_small"), ("lds_large_2000", "lds_large"), ("split_flop_20000", "split_flop"),
                                        ("split_ways_2", "split_flop"), ("split_ways_3", "split_flop")])
@pytest.mark.parametrize("step", [-1, 1])
def test_model_notices_each_moved_cut_moving_by_one(mode, const, step):
    cuts = mc.cuts_of(mc.MODES[mode])
    moved = {**cuts, const: cuts[const] + step}
    runs = [n for n in mc.NAMES if mode in mc.RUNS[n]]
    assert [n for n in runs if mc.expected_counts(mc.build(n), mode, moved) != mc.expected_counts(mc.build(n), mode)], f"{mode}: {const} {step:+d} goes unnoticed"


@pytest.mark.parametrize("name", mc.NAMES)
def test_reference_gives_hits_and_identities_where_a_row_is_meant_to_show_both(name):
    c = mc.build(name)
    mrp = c.mask[0]
    want, hit = _ref(name, "plus_times")
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2.0 ** 53
    absA, absB = (c.A[0], c.A[1], np.abs(c.A[2])), (c.B[0], c.B[1], np.abs(c.B[2]))
    assert masked_ref.spgemm_masked(absA, absB, c.M, c.N, c.mask, "plus_times")[0].max() < 2.0 ** 53, "every partial sum in any order is an exact integer"
    assert np.all(want[~hit] == 0.0)
    claims = 0
    for i, r in enumerate(c.rows):
        h = hit[mrp[i]:mrp[i + 1]]
        if r.hits == "both":
            assert h.any() and not h.all(), r.tag
        elif r.hits == "all":
            assert h.all() and h.size, r.tag
        elif r.hits == "none":
            assert not h.any() and h.size, r.tag
        claims += r.hits != ""
    assert claims >= 1 or name.startswith("open_")
    assert c.M == 1 or (hit.any() and not hit.all())
    for s in c.semirings[1:]:
        v, h = _ref(name, s)
        assert np.array_equal(h, hit) and np.all(v[~h] == mc.IDENTITY[s]) and np.isfinite(v[h]).all(), "a stray identity would show"
    if name == "split_mlen_1024":                                      # +k and −k alone: hits whose plus-times value is exactly 0.0
        for tag in ("flop_2p20", "flop_2p20_plus_1"):
            i = [r.tag for r in c.rows].index(tag)
            cols = c.mask[1][mrp[i]:mrp[i + 1]]
            for z in (3001, 3002):
                k = mrp[i] + int(np.searchsorted(cols, z))
                assert c.mask[1][k] == z and hit[k] and want[k] == 0.0
                assert _ref(name, "min_plus")[0][k] != np.inf
            assert not hit[mrp[i]:mrp[i + 1]][cols >= 3100].any(), "slots that receive nothing"
        # the two products of column 3002 sit in the first and in the last tile of 256 entries of A: two parts of the split row
        i = [r.tag for r in c.rows].index("flop_2p20_plus_1")
        arow = c.A[1][c.A[0][i]:c.A[0][i + 1]]
        holds = [pos for pos, bq in enumerate(arow) if 3002 in c.B[1][c.B[0][bq]:c.B[0][bq + 1]]]
        assert [p // mc.WG for p in holds] == [0, 3]
        holds = [pos for pos, bq in enumerate(arow) if 3001 in c.B[1][c.B[0][bq]:c.B[0][bq + 1]]]
        assert [p // mc.WG for p in holds] == [0, 0]


def test_wave_kernel_rows_stand_where_they_claim():
    """the rows of wave_tiles, from the arrays: where the empty rows of B sit in the tiles of 64, what a tile's products add up to, where the products fall
    against the mask row"""
    c = mc.build("wave_tiles")
    blen = np.diff(c.B[0])
    tags = [r.tag for r in c.rows]

    def parts(tag):
        i = tags.index(tag)
        arow = c.A[1][c.A[0][i]:c.A[0][i + 1]]
        cols = np.concatenate([c.B[1][c.B[0][p]:c.B[0][p + 1]] for p in arow] + [np.zeros(0, np.int32)])
        return blen[arow], cols, c.mask[1][c.mask[0][i]:c.mask[0][i + 1]]

    deg, _, _ = parts("empty_b_first_mid_last_of_tile")
    assert len(deg) == 64 and [k for k in range(64) if deg[k] == 0] == [0, 31, 63]
    tile_sums = lambda tag: [int(parts(tag)[0][k:k + mc.WAVE_TILE].sum()) for k in range(0, len(parts(tag)[0]), mc.WAVE_TILE)]
    assert tile_sums("tile_0_all_empty") == [0, 64] and tile_sums("tile_1_all_empty") == [64, 0] and tile_sums("tile_1_of_3_all_empty") == [64, 0, 2]
    assert [tile_sums(f"tile_total_{f}") for f in (64, 65, 128, 129)] == [[64], [65], [128], [129]]
    assert tile_sums("na_65") == [64, 1] and tile_sums("na_128") == [64, 64] and tile_sums("na_129") == [64, 64, 1]
    _, cols, mask = parts("all_below_the_mask")
    assert cols.max() < mask.min()
    for tag, mlen in (("all_above_the_mask_pad", 40), ("all_above_the_mask_63", 63), ("all_above_the_mask_64", 64)):
        _, cols, mask = parts(tag)
        assert cols.min() > mask.max() and len(mask) == mlen
    for mlen in (63, 64):
        _, cols, mask = parts(f"first_and_last_column_m{mlen}")
        assert list(cols) == [mask[0], mask[-1]] and len(mask) == mlen
    for tag in ("column_n_minus_1", "column_n_minus_1_m64"):
        _, cols, mask = parts(tag)
        assert c.N - 1 in cols and mask[-1] == c.N - 1
    r = mc.build("row256")
    i = [x.tag for x in r.rows].index("clip_edges")
    mask = r.mask[1][r.mask[0][i]:r.mask[0][i + 1]]
    brow = r.A[1][r.A[0][i]]
    assert list(r.B[1][r.B[0][brow]:r.B[0][brow + 1]]) == [mask[0] - 1, mask[0], mask[-1], mask[-1] + 1], "cmin − 1, cmin, cmax, cmax + 1"


def test_triangle_graphs_of_the_gpu_test():
    """the graphs of the triangle tests are what they claim, and the model applied to L gives the classes they are built for"""
    d = mc.cuts_of({})
    for k in (65, 66, 67):
        rp, ci = mc.graph_csr(*mc.clique(k))
        mlen, flop = mc.lower_rows(rp, ci)
        assert mlen.max() == k - 1 and flop.max() == (k - 1) * (k - 2) // 2 <= mc.WAVE_FLOP
        assert mc.counts_of(mlen, flop, d)["lds_small"] == max(0, k - 1 - mc.WAVE_MASK) and mc.counts_of(mlen, flop, d)["skip"] == 2
    n, edges, extra = mc.rows_with_products()
    mlen, flop = mc.lower_rows(*mc.graph_csr(n, edges))
    assert list(flop[extra]) == [4095, 4096, 4097] and mlen[extra].max() <= mc.WAVE_MASK
    assert [mc.row_class(mlen[v], flop[v], d) for v in extra] == ["wave", "wave", "lds_small"]
    for h, cls in ((1024, "lds_small"), (1025, "lds_large"), (8192, "lds_large"), (8193, "global")):
        n, edges = mc.hub_over_ring(h)
        mlen, flop = mc.lower_rows(*mc.graph_csr(n, edges))
        assert (mlen[h], flop[h]) == (h, h) and mc.row_class(mlen[h], flop[h], d) == cls
        n, edges = mc.hub_over_ring(h, 24)
        mlen, flop = mc.lower_rows(*mc.graph_csr(n, edges))
        assert mlen[h] == h and flop[h] == 24 * h > 20000
        assert mc.row_class(mlen[h], flop[h], mc.cuts_of(mc.MODES["split_flop_20000"])) == ("split_lds" if h <= 1024 else "split_global")
