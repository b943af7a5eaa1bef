"""Inputs for SpGEMM (g4s_amd/csrc/spgemm.hip) whose rows sit ON the limits of its row classes — the symbolic classes by product bound, the numeric classes
by output length, the one-wavefront kernel's hand-back, the long-B list, the rank kernel's chunk sizes, the clip of the bound at B's width — plus a numpy
restatement of the classification and of the two histogram lines the library prints under G4S_DEBUG. numpy only: no GPU, no torch.

Every edge is a pair of rows, "at" the limit and "just past" it, inside one product with ordinary rows around them. Values are integers of [−4, 4], exact zeros
kept: every plus-times sum is exact in fp64 in any order, min, max and or are exact by contract, so every comparison of these cases is bit for bit.

tests/test_spgemm_cases_cpu.py proves that every row has the product, output and entry count its name claims, that the pairs fall into the neighbouring
classes, and that the union covers every limit (COVERAGE); tests/test_spgemm_classes_gpu.py runs them and compares C and both histogram lines."""
import functools
from typing import NamedTuple

import numpy as np

# ---- the limits, each beside the source line it mirrors (g4s_amd/csrc/spgemm.hip unless another file is named)
SYM_LIMITS = (32, 512, 4096, 32768, 2097152)     # `constexpr ClassLimits kSymLimits{{32, 512, G4S_SPGEMM_SYM_MEDIUM, 32768, 2097152, -1}, {0, 0, 0, 1, 1, 0}};`
SYM_RAW = (False, False, False, True, True)      # … its second brace: the last two limits look at the unclipped bound; the sixth (−1) takes no row
NUM_LIMITS = (32, 512, 1024, 2048, 4096, 1048576)   # `constexpr ClassLimits kNumLimits{{32, 512, 1024, 2048, 4096, G4S_SPGEMM_BIG_LIMIT}, …};`
NUM_LIMIT_RANK = 8192                            # num_classing: `c.fifth_limit = c.rank && windows_take(sw, pre->cmap.width(N), 4) ? 8192 : kNumLimits.lim[4];`
SMALL_CAP = 512                                  # `constexpr int kSmallCap = 512;` — spgemm_small_wave_kernel: `if (na > 64 || flop > CAP)` hands the row back
TINY_CAP = 64                                    # `constexpr int kTinyCap = 64;` — the same test in the form that takes the symbolic tiny class
LANES = 64                                       # … and its `na > 64`: one lane per A-entry
LONG_CAP = 255                                   # `constexpr int kLongCap = 255;` — defer_long_b: `if (slot >= kLongCap) return false;`
WINDOW_MAX_N = 4 << 20                           # `constexpr int kWindowMaxN = 4 << 20;`
RANK_CHUNK = 8192                                # spgemm_rank.hpp: `constexpr int kRankChunk = G4S_SPGEMM_RANK_PER * kRankT;` = 8 · 1024
RANK_SMALL_CAP = 2000                            # spgemm_rank.hpp: `constexpr int kRankSmallT = 512, kRankSmallCap = 2000;`
M3_CUT = 8192                                    # `kNumM3Cut = 8192`: with G4S_SPGEMM_T_NUM_M3 the rows of (0, cut] outputs take that shape, the rest 1 024 threads


def long_b_threshold(threads):
    """`return threads >= 256 ? threads / 4 : 1 << 30;` — a B row of MORE entries is deferred to the workgroup (`if (b1 - b0 <= threshold) return false;`)"""
    return threads // 4 if threads >= 256 else 1 << 30


def window_chunk(threads):
    """`static constexpr int kChunk = 8 * T;` — outputs per value pass of the window kernels (256 threads: 2 048)"""
    return 8 * threads


SYM_CLASSES = ("empty", "tiny", "small", "medium", "large", "window", "hub")
NUM_CLASSES = ("empty", "<=32", "<=512", "<=1024", "<=2048", "<=4096", "<=1M", "hub", "rank")
SEMIRINGS = ("plus_times", "min_plus", "max_plus", "or_and")


def sym_class(F, N):
    """The symbolic class of a row of F products against a B of N columns, from the documented rule: no products — empty; then the first limit the row's
    size fits under, where the size is min(F, N) for the limits 32, 512 and 4 096 and F itself for 32 768 and 2 097 152; past them all — hub."""
    if F == 0:
        return "empty"
    clipped = min(F, N)
    if clipped <= 32:
        return "tiny"
    if clipped <= 512:
        return "small"
    if clipped <= 4096:
        return "medium"
    if F <= 32768:
        return "large"
    if F <= 2097152:
        return "window"
    return "hub"


def num_class(Z, rank_on, m2_tables=False):
    """The numeric class of a row of Z outputs that carries no cuts. The fifth limit is 8 192 instead of 4 096 while the rank path is on and the window kernel
    takes that class (m2_tables: G4S_SPGEMM_MID_TABLES & 4 hands it to a key table that holds 4 096 entries)."""
    if Z == 0:
        return "empty"
    lim4 = NUM_LIMIT_RANK if rank_on and not m2_tables else 4096
    for name, lim in zip(NUM_CLASSES[1:7], (32, 512, 1024, 2048, lim4, 1048576)):
        if Z <= lim:
            return name
    return "hub"


# ------------------------------------------------------------------------------------------------ the modes of the GPU test
MODES = {
    "default": {},
    "no_wave_rows": {"G4S_SPGEMM_NO_WAVE_ROWS": "1"},
    "window_max_n_0": {"G4S_SPGEMM_WINDOW_MAX_N": "0"},
    "no_rank": {"G4S_SPGEMM_NO_RANK": "1"},
    "no_units": {"G4S_SPGEMM_NO_UNITS": "1"},
    "mid_tables_1": {"G4S_SPGEMM_MID_TABLES": "1"},
    "mid_tables_2": {"G4S_SPGEMM_MID_TABLES": "2"},
    "mid_tables_4": {"G4S_SPGEMM_MID_TABLES": "4"},
    "t_num_m3_256": {"G4S_SPGEMM_T_NUM_M3": "256"},
    "t_num_m3_256_no_rank": {"G4S_SPGEMM_T_NUM_M3": "256", "G4S_SPGEMM_NO_RANK": "1"},
}


class Row(NamedTuple):
    tag: str
    F: int                   # products
    Z: int                   # outputs
    na: int                  # entries of the A row


class Edge(NamedTuple):
    const: str               # the limit or cap the pair stands on (a key of COVERAGE)
    at: str                  # tag of the row at the limit
    past: str                # tag of the row just past it ("" where the limit has no far side in this case)
    phase: str               # "sym", "num" (rank off), "num_rank" (rank on), or "other" (no class change: a hand-back, a list, a chunk)
    at_cls: str = ""
    past_cls: str = ""


class Case(NamedTuple):
    name: str
    A: tuple                 # (rowptr int32, colids int32, values float64)
    B: tuple
    M: int
    K: int
    N: int
    rows: tuple              # Row per A row
    edges: tuple             # Edge…
    semirings: tuple


# ------------------------------------------------------------------------------------------------ builders
class _Build:
    """B from disjoint column blocks, prefixes of a block (exact remainders), single-entry rows (±1), empty rows and copies of a block (products without
    outputs); A rows as lists of B rows with the counts they are meant to have."""

    def __init__(self):
        self.brows, self.arows, self.rows, self.next_col = [], [], [], 0

    def _b(self, cols):
        self.brows.append(np.asarray(cols, np.int64))
        return len(self.brows) - 1

    def block(self, n):
        self.next_col += n
        return self._b(np.arange(self.next_col - n, self.next_col))

    def single(self):
        return self.block(1)

    def empty(self):
        return self._b(np.zeros(0, np.int64))

    def prefix(self, b, n):
        assert 0 < n <= len(self.brows[b])
        return self._b(self.brows[b][:n])

    def copy(self, b):
        return self._b(self.brows[b])

    def copies(self, b, n):
        return [self.copy(b) for _ in range(n)]

    def cols(self, cols):
        return self._b(np.sort(np.asarray(cols, np.int64)))

    def row(self, tag, brows, F, Z):
        brows = sorted(brows)
        assert len(set(brows)) == len(brows)
        self.arows.append(np.asarray(brows, np.int64))
        self.rows.append(Row(tag, int(F), int(Z), len(brows)))

    def ordinary(self, rng, n=6):
        """a few ordinary rows around the edges: short rows over B rows that exist already, their counts worked out here from the blocks themselves"""
        K = len(self.brows)
        for i in range(n):
            pick = sorted(int(x) for x in rng.choice(K, size=min(K, int(rng.integers(1, 5))), replace=False))
            F = sum(len(self.brows[b]) for b in pick)
            if F > 400:
                pick, F = pick[:1], len(self.brows[pick[0]])
            if F > 400:
                continue
            Z = len(np.unique(np.concatenate([self.brows[b] for b in pick]))) if F else 0
            self.row(f"ordinary_{i}", pick, F, Z)

    def finish(self, name, edges, seed, N=None, semirings=SEMIRINGS):
        rng = np.random.default_rng(seed)
        K, M = len(self.brows), len(self.arows)
        N = self.next_col if N is None else N
        assert N >= self.next_col and N <= WINDOW_MAX_N
        ints = lambda n: rng.integers(-4, 5, n).astype(np.float64)
        brp = np.concatenate([[0], np.cumsum([len(r) for r in self.brows])]).astype(np.int32)
        bci = (np.concatenate(self.brows) if K else np.zeros(0)).astype(np.int32)
        arp = np.concatenate([[0], np.cumsum([len(r) for r in self.arows])]).astype(np.int32)
        aci = (np.concatenate(self.arows) if M else np.zeros(0)).astype(np.int32)
        ava = ints(aci.size)
        few = np.repeat(np.diff(arp) < 8, np.diff(arp)) & (ava == 0)    # a zero in a row of a few entries would zero the whole row: those rows keep no zeros
        ava[few] = rng.choice([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0], int(few.sum()))
        A, B = (arp, aci, ava), (brp, bci, ints(bci.size))
        for a in A + B:
            a.setflags(write=False)
        tags = [r.tag for r in self.rows]
        assert len(set(tags)) == len(tags)
        return Case(name, A, B, M, K, N, tuple(self.rows), tuple(edges), tuple(semirings))


def _short(edge_rows):
    """Every row of at most 512 products — the one-call form's numeric phase reuses the symbolic lists — or, with edge_rows, the same plus a row of 513
    products (no reuse: the numeric line shows the numeric classes) and the rows that only the numeric classes tell apart."""
    b = _Build()
    b20, b12, b500 = b.block(20), b.block(12), b.block(500)
    one = b.single()
    empties = [b.empty() for _ in range(33)]                           # in front of the singles: the 65th entry of a row of 65 is then one of its own columns
    singles = [b.single() for _ in range(64)]
    b32, b33, b64, b512 = b.block(32), b.block(33), b.block(64), b.block(512)
    b.row("na_0", [], 0, 0)
    b.row("only_empty_b_rows", empties[:3], 0, 0)
    b.row("F_32", [b20, b12], 32, 32)
    b.row("F_33", [b20, b12, one], 33, 33)
    b.row("F_512", [b500, b12], 512, 512)
    b.row("tiny_na_64", singles[:31] + empties, 31, 31)               # 33 of the 64 entries point at empty B rows
    b.row("tiny_na_65", singles[:32] + empties, 32, 32)
    b.row("small_na_64", singles[:63] + [b12], 75, 75)
    b.row("small_na_65", singles[:64] + [b12], 76, 76)
    b.row("one_b_row_32", [b32], 32, 32)
    b.row("one_b_row_33", [b33], 33, 33)
    b.row("one_b_row_64", [b64], 64, 64)
    b.row("one_b_row_512", [b512], 512, 512)
    b.row("twice_b20", [b20, b.copy(b20)], 40, 20)                     # every output is a sum of two products
    edges = [Edge("sym_32", "F_32", "F_33", "sym", "tiny", "small"), Edge("sym_32", "one_b_row_32", "one_b_row_33", "sym", "tiny", "small"),
             Edge("sym_512", "F_512", "", "sym", "small"), Edge("sym_512", "one_b_row_512", "", "sym", "small"),
             Edge("lanes_64", "tiny_na_64", "tiny_na_65", "other"), Edge("lanes_64", "small_na_64", "small_na_65", "other"),
             Edge("small_cap_512", "F_512", "", "other"), Edge("empty", "na_0", "only_empty_b_rows", "other")]
    if edge_rows:
        b.row("F_513", [b500, b12, one], 513, 513)
        b.row("F_513_Z_512", [b500, b12, b.prefix(b500, 1)], 513, 512)  # numerically "<= 512", and handed back by the wave kernel for its products
        b.row("Z_32_F_52", [b20, b12, b.copy(b20)], 52, 32)
        b.row("Z_33_F_53", [b20, b12, one, b.copy(b20)], 53, 33)
        edges += [Edge("sym_512", "F_512", "F_513", "sym", "small", "medium"), Edge("num_512", "F_513_Z_512", "F_513", "num", "<=512", "<=1024"),
                  Edge("small_cap_512", "F_512", "F_513_Z_512", "other"), Edge("num_32", "Z_32_F_52", "Z_33_F_53", "num", "<=32", "<=512")]
    b.ordinary(np.random.default_rng(3))
    return b.finish("short_edge" if edge_rows else "short", edges, seed=11 + edge_rows, N=b.next_col + 40)


def _mid():
    b = _Build()
    b1024, b2048, b4096, b600, one = b.block(1024), b.block(2048), b.block(4096), b.block(600), b.single()
    b.row("Z_1024", [b1024], 1024, 1024)
    b.row("Z_1025", [b1024, one], 1025, 1025)
    b.row("Z_2048", [b2048], 2048, 2048)                               # one full chunk of the 256-thread window kernel
    b.row("Z_2049", [b2048, one], 2049, 2049)                          # … and one output in a second chunk
    b.row("F_4096", [b4096], 4096, 4096)
    b.row("F_4097", [b4096, one], 4097, 4097)                          # a rank row with a single chunk below 8 192 outputs
    b.row("F_4097_Z_600", [b600] + b.copies(b600, 5) + [b.prefix(b600, 497)], 4097, 600)   # a rank row whose output is short
    b.row("small_row", [b.block(40), one], 41, 41)
    b.ordinary(np.random.default_rng(4))
    edges = [Edge("num_1024", "Z_1024", "Z_1025", "num", "<=1024", "<=2048"), Edge("num_1024", "Z_1024", "Z_1025", "num_rank", "<=1024", "<=2048"),
             Edge("num_2048", "Z_2048", "Z_2049", "num", "<=2048", "<=4096"), Edge("num_2048", "Z_2048", "Z_2049", "num_rank", "<=2048", "<=4096"),
             Edge("window_chunk_2048", "Z_2048", "Z_2049", "other"),
             Edge("sym_4096", "F_4096", "F_4097", "sym", "medium", "large"), Edge("sym_4096", "F_4096", "F_4097_Z_600", "sym", "medium", "large"),
             Edge("num_4096", "F_4096", "F_4097", "num", "<=4096", "<=1M")]
    return b.finish("mid", edges, seed=21)


def _long():
    b = _Build()
    b4096 = [b.block(4096) for _ in range(8)]
    b2000, one, one2 = b.block(2000), b.single(), b.single()
    b.row("F_32768", b4096, 32768, 32768)
    b.row("F_32769", b4096 + [one], 32769, 32769)
    b.row("Z_8192_2000", b4096[:2] + [b2000], 10192, 10192)           # a rank row whose last chunk holds kRankSmallCap outputs
    b.row("Z_8192_2001", b4096[:2] + [b2000, one2], 10193, 10193)     # … and one more
    b.row("small_row", [b.block(40), one], 41, 41)
    b.ordinary(np.random.default_rng(5))
    edges = [Edge("sym_32768_raw", "F_32768", "F_32769", "sym", "large", "window"), Edge("rank_small_cap_2000", "Z_8192_2000", "Z_8192_2001", "other"),
             Edge("rank_chunk_8192", "F_32768", "F_32769", "other")]
    return b.finish("long", edges, seed=31)


def _hub():
    b = _Build()
    h0, h1 = b.block(524288), b.block(524288)
    c0, c1 = b.copy(h0), b.copy(h1)
    p1, one, b8191, s1, s2 = b.prefix(h0, 1), b.single(), b.block(8191), b.single(), b.single()
    four = [h0, h1, c0, c1]
    b.row("F_2097152", four, 2097152, 1048576)                        # symbolic: window — a rank row, or "<= 1M" with the rank path off
    b.row("F_2097153_Z_1048576", four + [p1], 2097153, 1048576)       # symbolic: hub; numeric: "<= 1M"
    b.row("F_2097153_Z_1048577", four + [one], 2097153, 1048577)      # hub in both phases
    b.row("Z_8191", [b8191], 8191, 8191)                               # rank rows; with the rank path off the M3 class on either side of its shape cut
    b.row("Z_8192", [b8191, s1], 8192, 8192)
    b.row("Z_8193", [b8191, s1, s2], 8193, 8193)
    b.row("small_row", [b.block(40), one], 41, 41)
    edges = [Edge("sym_2097152_raw", "F_2097152", "F_2097153_Z_1048576", "sym", "window", "hub"),
             Edge("num_1048576", "F_2097153_Z_1048576", "F_2097153_Z_1048577", "num", "<=1M", "hub"),
             Edge("num_1048576", "F_2097153_Z_1048576", "F_2097153_Z_1048577", "num_rank", "<=1M", "hub"),
             Edge("m3_cut_8192", "Z_8191", "Z_8192", "other"), Edge("m3_cut_8192", "Z_8192", "Z_8193", "other")]
    return b.finish("hub", edges, seed=41, semirings=("plus_times", "min_plus"))


def _hub_beside_rank(N):
    """One rank row beside symbolic hub rows (more than 2 097 152 products) of 4 096, 4 097 and 8 192 outputs — and of 8 193 with N = 8 193: the only rows
    without cuts that can hold more than 4 096 outputs while the rank path is on, i.e. the only ones that see the numeric limit move to 8 192."""
    b = _Build()
    lo, hi = b.block(4096), b.block(4096)
    heap = [lo] + b.copies(lo, 512)                                    # 513 · 4 096 = 2 101 248 products on 4 096 columns
    b.row("rank_row", [lo, hi], 8192, 8192)
    if N == 8192:
        b.row("hub_Z_4096", heap, 2101248, 4096)
        b.row("hub_Z_4097", heap + [b.prefix(hi, 1)], 2101249, 4097)
    b.row("hub_Z_8192", heap + [hi], 2105344, 8192)
    edges = [Edge("num_4096", "hub_Z_4096", "hub_Z_4097", "num", "<=4096", "<=1M"), Edge("num_8192_rank", "hub_Z_8192", "", "num_rank", "<=4096")]
    if N == 8193:
        b.row("hub_Z_8193", heap + [hi, b.single()], 2105345, 8193)
        edges = [Edge("num_8192_rank", "hub_Z_8192", "hub_Z_8193", "num_rank", "<=4096", "<=1M")]
    b.row("small_row", [b.prefix(lo, 40), b.prefix(hi, 1)], 41, 41)
    return b.finish(f"hub_beside_rank_{N}", edges, seed=51 + N % 2, N=N, semirings=("plus_times", "min_plus"))


def _clip_32():
    """N = 32: every bound clips to 32 — rows of 33, 64, 65 and 2 000 products are all "tiny". The tiny form of the wave kernel holds 64 products: the rows of
    33 and 64 stay with it, those of 65 and 2 000 are handed back to the table kernel."""
    b = _Build()
    b32 = b.block(32)
    cp = b.copies(b32, 62)
    b.row("F_33", [b32, b.prefix(b32, 1)], 33, 32)
    b.row("F_64", [b32, cp[0]], 64, 32)
    b.row("F_65", [b32, cp[0], b.prefix(b32, 1)], 65, 32)
    b.row("F_2000", [b32] + cp[:61] + [b.prefix(b32, 16)], 2000, 32)
    b.row("F_20", [b.prefix(b32, 20)], 20, 20)
    edges = [Edge("clip_at_cols", "F_33", "", "sym", "tiny"), Edge("clip_at_cols", "F_65", "", "sym", "tiny"), Edge("clip_at_cols", "F_2000", "", "sym", "tiny"),
             Edge("tiny_cap_64", "F_64", "F_65", "other")]
    return b.finish("clip_32", edges, seed=61, N=32)


def _clip_512():
    """N = 512: a row of 20 000 products over 300 B rows is "small". The wave kernel hands it back (300 entries); the table kernel defers the B rows of more
    than 64 entries to its long-B list: 282 of them, so the list is full at 255 and the other 27 are walked in their lane groups. The 64-entry rows sit on the
    threshold itself and are never deferred."""
    b = _Build()
    b.next_col = 512
    win = lambda start, n: (start + np.arange(n)) % 512
    r65 = [b.cols(win(7 * i, 65)) for i in range(280)]                 # 280 · 65 = 18 200; their union is every column
    r64 = [b.cols(win(29 * i, 64)) for i in range(18)]                 # 18 · 64 = 1 152
    r324 = [b.cols(win(100, 324)), b.cols(win(300, 324))]              # 648
    b.row("F_20000", r65 + r64 + r324, 20000, 512)
    b.row("deferred_255", r65[:255] + r64[:2], 255 * 65 + 128, 512)    # the list exactly full
    b.row("deferred_256", r65[:256] + r64[:2], 256 * 65 + 128, 512)    # one B row that finds no slot
    b.row("F_64", [r64[0]], 64, 64)
    edges = [Edge("clip_at_cols", "F_20000", "", "sym", "small"), Edge("long_cap_255", "deferred_255", "deferred_256", "other"),
             Edge("long_cap_255", "F_20000", "", "other"), Edge("long_b_threshold_64", "F_20000", "", "other")]
    return b.finish("clip_512", edges, seed=62, N=512)


def _clip_4096(N):
    """A row of more than 2 097 152 products on 4 096 columns: "medium" (every column set) at N = 4 096, hub at N = 4 097."""
    b = _Build()
    lo = b.block(4096)
    b.row("F_2101248", [lo] + b.copies(lo, 512), 2101248, 4096)
    b.row("small_row", [b.prefix(lo, 40)], 40, 40)
    edges = [Edge("clip_at_cols", "F_2101248", "", "sym", "medium" if N == 4096 else "hub")]
    return b.finish(f"clip_{N}", edges, seed=63, N=N, semirings=("plus_times", "min_plus"))


_BUILDERS = {
    "short": functools.partial(_short, False), "short_edge": functools.partial(_short, True), "mid": _mid, "long": _long, "hub": _hub,
    "hub_beside_rank_8192": functools.partial(_hub_beside_rank, 8192), "hub_beside_rank_8193": functools.partial(_hub_beside_rank, 8193),
    "clip_32": _clip_32, "clip_512": _clip_512, "clip_4096": functools.partial(_clip_4096, 4096), "clip_4097": functools.partial(_clip_4096, 4097),
}
NAMES = list(_BUILDERS)
BIG = ("hub", "hub_beside_rank_8192", "hub_beside_rank_8193", "clip_4096", "clip_4097")   # millions of products: plus-times and min-plus only


def semirings_of(name):
    """the semirings the GPU test runs the case over (known without building it)"""
    return SEMIRINGS[:2] if name in BIG else SEMIRINGS


@functools.lru_cache(maxsize=None)
def build(name):
    """The case (cached: its arrays are read-only)."""
    return _BUILDERS[name]()


def row(case, tag):
    return next(r for r in case.rows if r.tag == tag)


# ------------------------------------------------------------------------------------------------ which mode runs which case
# Each mode with the cases whose edges it moves: the short-row switch with the rows the wave kernel takes or hands back, the three switches that turn the rank
# path off (no window kernels, no rank, no unit lists) with the rows that carry cuts and the rows beside them, the key tables of the mid-size classes with the
# rows of those classes, the M3 shape with the case that holds M3 rows on both sides of its cut.
RUNS = {
    "short": ("default", "no_wave_rows"),
    "short_edge": ("default", "no_wave_rows"),
    "mid": ("default", "window_max_n_0", "no_rank", "no_units", "mid_tables_1", "mid_tables_2", "mid_tables_4"),
    "long": ("default", "window_max_n_0", "no_rank", "no_units"),
    "hub": ("default", "no_rank", "t_num_m3_256", "t_num_m3_256_no_rank"),
    "hub_beside_rank_8192": ("default", "no_rank", "no_units", "mid_tables_1", "mid_tables_2", "mid_tables_4"),
    "hub_beside_rank_8193": ("default", "mid_tables_4"),
    "clip_32": ("default", "no_wave_rows"),
    "clip_512": ("default", "no_wave_rows"),
    "clip_4096": ("default", "window_max_n_0", "mid_tables_1"),
    "clip_4097": ("default",),
}

# Every limit and cap against the cases that stand on it (an Edge of that case names it) and the modes that must run them.
COVERAGE = {
    "sym_32": [("short", "default"), ("short", "no_wave_rows")],
    "sym_512": [("short_edge", "default"), ("short_edge", "no_wave_rows")],
    "sym_4096": [("mid", "default"), ("mid", "mid_tables_1"), ("mid", "window_max_n_0")],
    "sym_32768_raw": [("long", "default"), ("long", "window_max_n_0"), ("long", "no_rank")],
    "sym_2097152_raw": [("hub", "default"), ("hub", "no_rank")],
    "num_32": [("short_edge", "default"), ("short_edge", "no_wave_rows")],
    "num_512": [("short_edge", "default"), ("short_edge", "no_wave_rows")],
    "num_1024": [("mid", "default"), ("mid", "mid_tables_1"), ("mid", "no_rank")],
    "num_2048": [("mid", "default"), ("mid", "mid_tables_2"), ("mid", "no_units")],
    "num_4096": [("mid", "no_rank"), ("mid", "window_max_n_0"), ("hub_beside_rank_8192", "no_rank"), ("hub_beside_rank_8192", "mid_tables_4")],
    "num_8192_rank": [("hub_beside_rank_8192", "default"), ("hub_beside_rank_8193", "default"), ("hub_beside_rank_8193", "mid_tables_4")],
    "num_1048576": [("hub", "default"), ("hub", "no_rank")],
    "small_cap_512": [("short", "default"), ("short_edge", "default")],
    "tiny_cap_64": [("clip_32", "default")],
    "lanes_64": [("short", "default"), ("short_edge", "default")],
    "long_cap_255": [("clip_512", "default"), ("clip_512", "no_wave_rows")],
    "long_b_threshold_64": [("clip_512", "default"), ("clip_512", "no_wave_rows")],
    "rank_chunk_8192": [("long", "default")],
    "rank_small_cap_2000": [("long", "default")],
    "window_chunk_2048": [("mid", "default"), ("mid", "no_rank")],
    "m3_cut_8192": [("hub", "t_num_m3_256"), ("hub", "t_num_m3_256_no_rank")],
    "clip_at_cols": [("clip_32", "default"), ("clip_512", "default"), ("clip_4096", "default"), ("clip_4097", "default")],
    "empty": [("short", "default")],
}


# ------------------------------------------------------------------------------------------------ the two histogram lines
def rank_on(case, mode):
    """The rank path is on iff the symbolic phase has a large or window row, B is within the window kernels' width, the unit lists are on and
    G4S_SPGEMM_NO_RANK is unset."""
    env = MODES[mode]
    long_rows = any(sym_class(r.F, case.N) in ("large", "window") for r in case.rows)
    width_ok = case.N <= int(env.get("G4S_SPGEMM_WINDOW_MAX_N", WINDOW_MAX_N))   # (N2 <= N: the column map only narrows B)
    return long_rows and width_ok and "G4S_SPGEMM_NO_UNITS" not in env and "G4S_SPGEMM_NO_RANK" not in env


def expected_histograms(case, mode, one_call):
    """(symbolic, numeric): what the `g4s symbolic classes:` and `g4s numeric classes:` lines must count, as dicts keyed by SYM_CLASSES / NUM_CLASSES."""
    env = MODES[mode]
    sym = dict.fromkeys(SYM_CLASSES, 0)
    for r in case.rows:
        sym[sym_class(r.F, case.N)] += 1
    num = dict.fromkeys(NUM_CLASSES, 0)
    only_short = sym["medium"] + sym["large"] + sym["window"] + sym["hub"] == 0
    if one_call and only_short:                                        # the numeric phase takes the symbolic lists (sym_rc_valid): it prints their counts
        num["empty"], num["<=32"], num["<=512"] = sym["empty"], sym["tiny"], sym["small"]
        return sym, num
    rank = rank_on(case, mode)
    m2_tables = bool(int(env.get("G4S_SPGEMM_MID_TABLES", "0")) & 4)
    for r in case.rows:
        if rank and sym_class(r.F, case.N) in ("large", "window"):    # the rank rows are exactly the rows that wrote cuts
            num["rank"] += 1
        else:
            num[num_class(r.Z, rank, m2_tables)] += 1
    return sym, num
