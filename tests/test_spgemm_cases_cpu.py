"""The cases of tests/spgemm_cases.py are what their names claim: every row has exactly the products, outputs and entries it declares (counted here from the
index arrays and from tests/semiring_ref.py, not by the builders), the "at" and "just past" rows of every pair fall into the two neighbouring classes, every
limit and cap is stood on by a case that a mode of the GPU test runs (COVERAGE), the plus-times results are exact integers, and the other semirings would
show a stray identity or a stray 0.0. No GPU."""
import functools

import numpy as np
import pytest

from tests import semiring_ref
from tests import spgemm_cases as sc


@functools.lru_cache(maxsize=None)
def _ref(name, semiring):
    c = sc.build(name)
    out = semiring_ref.spgemm(c.A, c.B, c.M, semiring)
    for a in out:
        a.setflags(write=False)
    return out


def _counts(c):
    arp, aci, _ = c.A
    brp = c.B[0].astype(np.int64)
    na = np.diff(arp).astype(np.int64)
    F = np.zeros(c.M, np.int64)
    np.add.at(F, np.repeat(np.arange(c.M), na), np.diff(brp)[aci])
    return F, na


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_well_formed_and_every_row_has_its_declared_counts(name):
    c = sc.build(name)
    (arp, aci, ava), (brp, bci, bva) = c.A, c.B
    assert arp.dtype == brp.dtype == aci.dtype == bci.dtype == np.int32 and ava.dtype == bva.dtype == np.float64
    assert len(arp) == c.M + 1 and len(brp) == c.K + 1 and arp[0] == brp[0] == 0 and arp[-1] == len(aci) == len(ava) and brp[-1] == len(bci) == len(bva)
    assert len(c.rows) == c.M and c.N <= sc.WINDOW_MAX_N and c.semirings == sc.semirings_of(name)
    for rp, ci, width in ((arp, aci, c.K), (brp, bci, c.N)):
        assert np.all(np.diff(rp) >= 0) and (len(ci) == 0 or (ci.min() >= 0 and ci.max() < width))
        up = np.ones(len(ci), bool)
        up[1:] = np.diff(ci.astype(np.int64)) > 0
        up[rp[:-1][rp[:-1] < len(ci)]] = True
        assert up.all(), "sorted distinct columns in every row"
    for v in (ava, bva):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 4 and (v > 0).any() and (v < 0).any()
    assert (bva == 0).any(), "exact zeros are kept (in A only in rows of eight entries or more: a zero would blank a shorter row)"
    F, na = _counts(c)
    Z = np.diff(_ref(name, "plus_times")[0])
    for i, r in enumerate(c.rows):
        assert (r.F, r.Z, r.na) == (F[i], Z[i], na[i]), (r, F[i], Z[i], na[i])
    assert 0 < F.sum() < 8_000_000, "the reference multiplies a case in about a second"


def _cls(c, tag, phase):
    r = sc.row(c, tag)
    return sc.sym_class(r.F, c.N) if phase == "sym" else sc.num_class(r.Z, phase == "num_rank")


@pytest.mark.parametrize("name", sc.NAMES)
def test_at_and_past_rows_fall_into_neighbouring_classes(name):
    c = sc.build(name)
    assert c.edges
    for e in c.edges:
        assert e.const in sc.COVERAGE, e
        if e.phase == "other":
            continue
        order = sc.SYM_CLASSES if e.phase == "sym" else sc.NUM_CLASSES
        assert _cls(c, e.at, e.phase) == e.at_cls, e
        if e.past:
            assert _cls(c, e.past, e.phase) == e.past_cls, e
            assert order.index(e.past_cls) == order.index(e.at_cls) + 1, e


def test_class_rules_at_every_limit():
    """sym_class and num_class on either side of every limit, with and without the clip and the rank path"""
    wide = 1 << 22
    for lim, (lo, hi) in zip(sc.SYM_LIMITS, zip(sc.SYM_CLASSES[1:], sc.SYM_CLASSES[2:])):
        assert (sc.sym_class(lim, wide), sc.sym_class(lim + 1, wide)) == (lo, hi)
    for lim, raw, (lo, hi) in zip(sc.SYM_LIMITS, sc.SYM_RAW, zip(sc.SYM_CLASSES[1:], sc.SYM_CLASSES[2:])):
        assert sc.sym_class(lim + 1, lim) == (hi if raw else lo), "a B of exactly `lim` columns clips the bound for the first three limits only"
    assert sc.sym_class(0, 5) == "empty" and sc.sym_class(10 ** 9, 32) == "tiny" and sc.sym_class(10 ** 9, 33) == "small" and sc.sym_class(10 ** 9, 512) == "small"
    assert sc.sym_class(2097152, 4096) == "medium" and sc.sym_class(2097153, 4096) == "medium" and sc.sym_class(2097153, 4097) == "hub"
    assert sc.sym_class(32768, 4097) == "large" and sc.sym_class(32769, 4097) == "window"      # the raw limits are not clipped
    for lim, (lo, hi) in zip(sc.NUM_LIMITS, zip(sc.NUM_CLASSES[1:], sc.NUM_CLASSES[2:])):
        assert (sc.num_class(lim, False), sc.num_class(lim + 1, False)) == (lo, hi)
    assert [sc.num_class(z, True) for z in (4096, 4097, 8192, 8193)] == ["<=4096", "<=4096", "<=4096", "<=1M"]
    assert [sc.num_class(z, True, m2_tables=True) for z in (4096, 4097, 8192)] == ["<=4096", "<=1M", "<=1M"]
    assert sc.long_b_threshold(256) == 64 and sc.long_b_threshold(1024) == 256 and sc.long_b_threshold(64) == 1 << 30 and sc.window_chunk(256) == 2048


def _deferred(c, tag, threads=256):
    """how many B rows of the A row are longer than the long-B threshold of the table kernel that takes it"""
    i = [r.tag for r in c.rows].index(tag)
    blen = np.diff(c.B[0].astype(np.int64))[c.A[1][c.A[0][i]:c.A[0][i + 1]]]
    return int((blen > sc.long_b_threshold(threads)).sum()), int((blen == sc.long_b_threshold(threads)).sum())


def test_the_edges_without_a_class_change_stand_where_they_claim():
    for name in sc.NAMES:
        c = sc.build(name)
        for e in (e for e in c.edges if e.phase == "other"):
            at, past = sc.row(c, e.at), (sc.row(c, e.past) if e.past else None)
            if e.const == "lanes_64":
                assert (at.na, past.na) == (sc.LANES, sc.LANES + 1) and sc.sym_class(at.F, c.N) == sc.sym_class(past.F, c.N) and past.F <= sc.SMALL_CAP
                if e.at.startswith("tiny"):
                    assert past.F <= 32 and at.na - at.F >= 33, "at least 33 entries point at empty B rows"
            elif e.const == "small_cap_512":
                assert at.F == sc.SMALL_CAP and at.na <= sc.LANES and (past is None or (past.F == sc.SMALL_CAP + 1 and past.Z <= 512 and past.na <= sc.LANES))
            elif e.const == "tiny_cap_64":
                assert (at.F, past.F) == (sc.TINY_CAP, sc.TINY_CAP + 1) and sc.sym_class(past.F, c.N) == "tiny" and max(at.na, past.na) <= sc.LANES
            elif e.const == "empty":
                assert at.na == 0 and past.na > 0 and at.F == past.F == 0
            elif e.const == "long_cap_255":
                assert at.na > sc.LANES and sc.sym_class(at.F, c.N) == "small", "handed back to the 256-thread table kernel, in both phases"
                if past:
                    assert (_deferred(c, e.at)[0], _deferred(c, e.past)[0]) == (sc.LONG_CAP, sc.LONG_CAP + 1)
                else:
                    assert _deferred(c, e.at)[0] >= 282
            elif e.const == "long_b_threshold_64":
                assert _deferred(c, e.at)[1] >= 1 and _deferred(c, e.at)[0] >= 1
            elif e.const == "rank_small_cap_2000":
                assert (at.Z - sc.RANK_CHUNK, past.Z - sc.RANK_CHUNK) == (sc.RANK_SMALL_CAP, sc.RANK_SMALL_CAP + 1)
                assert all(sc.sym_class(r.F, c.N) == "large" for r in (at, past))
            elif e.const == "rank_chunk_8192":
                assert at.Z % sc.RANK_CHUNK == 0 and past.Z % sc.RANK_CHUNK == 1 and sc.sym_class(at.F, c.N) in ("large", "window")
            elif e.const == "window_chunk_2048":
                assert (at.Z, past.Z) == (sc.window_chunk(256), sc.window_chunk(256) + 1) and sc.sym_class(past.F, c.N) == "medium"
            elif e.const == "m3_cut_8192":
                assert past.Z == at.Z + 1 and sc.M3_CUT in (at.Z, past.Z) and sc.num_class(at.Z, False) == sc.num_class(past.Z, False) == "<=1M"
            else:
                raise AssertionError(f"no check for {e}")


def test_every_limit_is_covered_by_a_case_that_a_mode_runs():
    named = {(e.const, name) for name in sc.NAMES for e in sc.build(name).edges}
    wanted = {"sym_32", "sym_512", "sym_4096", "sym_32768_raw", "sym_2097152_raw", "num_32", "num_512", "num_1024", "num_2048", "num_4096", "num_8192_rank",
              "num_1048576", "small_cap_512", "tiny_cap_64", "lanes_64", "long_cap_255", "long_b_threshold_64", "rank_chunk_8192", "rank_small_cap_2000",
              "window_chunk_2048", "clip_at_cols"}
    assert wanted <= set(sc.COVERAGE)
    for const, runs in sc.COVERAGE.items():
        assert runs, const
        for name, mode in runs:
            assert (const, name) in named, f"{name} has no edge on {const}"
            assert mode in sc.RUNS[name] and mode in sc.MODES, (const, name, mode)
    assert set(sc.RUNS) == set(sc.NAMES) and all("default" in m for m in sc.RUNS.values())
    assert {m for modes in sc.RUNS.values() for m in modes} == set(sc.MODES), "a mode that no case runs"
    # both sides of every limit that has two: some case holds a pair across it
    two_sided = {e.const for name in sc.NAMES for e in sc.build(name).edges if e.past}
    assert set(sc.COVERAGE) - two_sided == {"clip_at_cols", "long_b_threshold_64"}
    # the clip: the same row is "medium" at N = 4 096 and hub at N = 4 097
    a, b = sc.build("clip_4096"), sc.build("clip_4097")
    assert a.rows == b.rows and (a.N, b.N) == (4096, 4097)


def test_expected_histograms_of_the_model():
    """the model on the cases whose lines are easy to count by hand"""
    c = sc.build("hub_beside_rank_8192")
    zero = lambda keys, **kw: {**dict.fromkeys(keys, 0), **kw}
    sym = zero(sc.SYM_CLASSES, small=1, large=1, hub=3)
    assert sc.expected_histograms(c, "default", True) == (sym, zero(sc.NUM_CLASSES, **{"<=512": 1, "<=4096": 3, "rank": 1}))
    assert sc.expected_histograms(c, "mid_tables_4", False) == (sym, zero(sc.NUM_CLASSES, **{"<=512": 1, "<=4096": 1, "<=1M": 2, "rank": 1}))
    assert sc.expected_histograms(c, "no_rank", True) == (sym, zero(sc.NUM_CLASSES, **{"<=512": 1, "<=4096": 1, "<=1M": 3}))
    assert sc.expected_histograms(c, "no_units", True)[1] == sc.expected_histograms(c, "no_rank", True)[1]
    s = sc.build("short")
    sym, num = sc.expected_histograms(s, "default", True)
    assert (num["empty"], num["<=32"], num["<=512"]) == (sym["empty"], sym["tiny"], sym["small"]) and sum(num.values()) == s.M
    num2 = sc.expected_histograms(s, "default", False)[1]
    assert num2 != num and sum(num2.values()) == s.M, "the two-call form classifies by outputs: the row of 40 products for 20 outputs moves"
    for name in sc.NAMES:
        for mode in sc.RUNS[name]:
            for one_call in (True, False):
                sym, num = sc.expected_histograms(sc.build(name), mode, one_call)
                assert sum(sym.values()) == sum(num.values()) == sc.build(name).M
    h = sc.build("hub")
    assert sc.expected_histograms(h, "default", True)[1]["rank"] == 4 and sc.expected_histograms(h, "t_num_m3_256_no_rank", True)[1]["<=1M"] == 5


@pytest.mark.parametrize("name", sc.NAMES)
def test_results_are_exact_and_would_show_a_stray_identity_or_zero(name):
    c = sc.build(name)
    pt = _ref(name, "plus_times")
    assert np.array_equal(pt[2], np.round(pt[2])) and np.abs(pt[2]).max() < 2.0 ** 53
    # Σ|a·b| per output bounds every partial sum in any order: exact integers below 2^53 on the way, too
    absA, absB = (c.A[0], c.A[1], np.abs(c.A[2])), (c.B[0], c.B[1], np.abs(c.B[2]))
    assert semiring_ref.spgemm(absA, absB, c.M, "plus_times")[2].max() < 2.0 ** 53
    refs = {s: _ref(name, s) for s in c.semirings}
    for s, (rp, ci, v) in refs.items():
        assert np.array_equal(rp, pt[0]) and np.array_equal(ci, pt[1]) and np.isfinite(v).all(), "one pattern; no identity survives in a stored entry"
    edge_tags = {t for e in c.edges for t in (e.at, e.past) if t}
    for i, r in enumerate(c.rows):
        if r.tag not in edge_tags or r.Z < 16 or r.F != r.Z:
            continue                                                   # (an output fed by hundreds of products has the extreme sum of [-8, 8] whatever happens)
        lo, hi = pt[0][i], pt[0][i + 1]
        for s in c.semirings[:3]:                                      # (one A value may feed the whole row: its sign is the row's, so only variety is asked per row)
            assert len(np.unique(refs[s][2][lo:hi])) >= 3, f"{r.tag}: {s} gives the row fewer than three different values"
        assert not np.array_equal(refs["min_plus"][2][lo:hi], pt[2][lo:hi])
    for s, want in (("min_plus", lambda v: (v > 0).any() and (v == 0).any()), ("max_plus", lambda v: (v < 0).any() and (v == 0).any()),
                    ("or_and", lambda v: set(np.unique(v)) == {0.0, 1.0})):
        assert s not in refs or want(refs[s][2]), f"{s}: no output of the case would show a stray 0.0"
    # the "at" and the "past" row of a pair differ in every semiring: the extra product changes an output or adds one
    for e in (e for e in c.edges if e.past):
        i, j = ([r.tag for r in c.rows].index(t) for t in (e.at, e.past))
        for s, (rp, ci, v) in refs.items():
            a = (ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]])
            b = (ci[rp[j]:rp[j + 1]], v[rp[j]:rp[j + 1]])
            if (s == "or_and" and len(a[0]) == len(b[0])) or len(a[0]) == len(b[0]) == 0:
                continue                                               # (an extra product on an existing output need not flip an or)
            assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), (e, s)
