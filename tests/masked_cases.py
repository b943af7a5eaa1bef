"""Inputs for the masked SpGEMM and for triangle counting (g4s_amd/csrc/spgemm_masked.hip) whose rows sit ON the limits of its seven row classes — the wave
class's 64 mask entries and 4 096 products, the 1 024- and 8 192-entry LDS tables, the 2^20 products above which a row is split — and on the edges the kernels
have of their own (tiles of 64 / 256 / 1 024 entries of A, the INT_MAX pad of the 64-slot mask row, the [cmin, cmax] clip, the split rows' parts and rounds, the
fold that skips identities), plus a numpy restatement of the classification, of the line the library prints under G4S_DEBUG and of g4s_masked_info.
numpy only: no GPU, no torch.

Every cut is a pair of rows, "at" the limit and "just past" it, inside one product with ordinary rows around them. Values are integers of [−4, 4], exact zeros
kept: every plus-times sum is exact in fp64 in any order, min, max and or are exact by contract, so every comparison of these cases is bit for bit.

tests/test_masked_cases_cpu.py proves that every row has the mask length, entry count and product count its descriptor claims, that the pairs fall into the
neighbouring classes, and that the union covers every edge (COVERAGE); tests/test_spgemm_masked_limits_gpu.py runs them and compares cval, the debug line and
g4s_masked_info."""
import functools
from typing import NamedTuple

import numpy as np

# ---- the limits, each beside the source line it mirrors (g4s_amd/csrc/spgemm_masked.hip)
WAVE_MASK = 64                                   # `constexpr int kWaveMask = 64;               // the wave class keeps one mask column per lane`
WAVE_FLOP = 4096                                 # `constexpr long long kWaveFlop = 4096;`
LDS_SMALL, LDS_LARGE = 1024, 8192                # `constexpr int kLdsSmall = 1024, kLdsLarge = 8192;`
SPLIT_FLOP = 1 << 20                             # `constexpr long long kSplitFlop = 1ll << 20;`
SPLIT_WAYS = 128                                 # `constexpr int kSplitWays = 128;`
WG = 256                                         # `constexpr int WG = 256;` — the tile of A entries of the small-table, global and split kernels
WG_LARGE = 1024                                  # `constexpr int kWgLarge = 1024;              // threads of the workgroup that holds a large table`
OPEN_LPR = 8                                     # `constexpr int kOpenLpr = 8;                 // lanes per row in the opening pass`
OPEN_ROWS_PER_WG = WG // OPEN_LPR                # `const int rows_per_wg = WG / kOpenLpr;` = 32; tc_lower_kernel's grid is `n / rows_per_wg + 1`
WAVE_ROWS_PER_WG = WG // 64                      # mk_wave_kernel: `const long long idx = (long long)blockIdx.x * (WG / 64) + wave;` = 4 rows per workgroup
WAVE_TILE = 64                                   # mk_wave_kernel: `for (int a0 = ab; a0 < ae; a0 += 64)`

CLASSES = ("skip", "wave", "lds_small", "lds_large", "global", "split_lds", "split_global")   # `enum { C_SKIP = 0, C_WAVE, C_LDS_S, C_LDS_L, C_GLOBAL, …`
SEMIRINGS = ("plus_times", "min_plus", "max_plus", "or_and")
IDENTITY = {"plus_times": 0.0, "min_plus": np.inf, "max_plus": -np.inf, "or_and": 0.0}

# ------------------------------------------------------------------------------------------------ the modes of the GPU test
MODES = {
    "default": {},
    "wave_flop_100": {"G4S_MASKED_WAVE_FLOP": "100"},
    "lds_small_100": {"G4S_MASKED_LDS_SMALL": "100"},
    "lds_large_2000": {"G4S_MASKED_LDS_LARGE": "2000"},
    "split_flop_20000": {"G4S_MASKED_SPLIT_FLOP": "20000"},
    "split_ways_2": {"G4S_MASKED_SPLIT_FLOP": "20000", "G4S_MASKED_SPLIT_WAYS": "2"},
    "split_ways_3": {"G4S_MASKED_SPLIT_FLOP": "20000", "G4S_MASKED_SPLIT_WAYS": "3"},
    "lds_small_0": {"G4S_MASKED_LDS_SMALL": "0"},
    "lds_large_0": {"G4S_MASKED_LDS_LARGE": "0"},
    "lds_over": {"G4S_MASKED_LDS_SMALL": "4000", "G4S_MASKED_LDS_LARGE": "100000"},   # above the tables: must clamp back to 1 024 and 8 192
}


def _env(env, name, default, lo, hi):
    """`if (!e || !*e) return dflt; return std::max(lo, std::min(hi, atoll(e)));`"""
    e = env.get(name, "")
    return default if e == "" else max(lo, min(hi, int(e)))


def cuts_of(env):
    """The effect of the five G4S_MASKED_* variables (read_cuts, clamps included): the wave class's products within [0, 2^30], the split threshold at least 1,
    the two LDS tables only downwards from 1 024 and 8 192, the parts of a split row within [2, 4 096]. `wave_mask` is no variable: it is here so that the
    sensitivity check can move it."""
    return {"wave_mask": WAVE_MASK,
            "wave_flop": _env(env, "G4S_MASKED_WAVE_FLOP", WAVE_FLOP, 0, 1 << 30),
            "split_flop": _env(env, "G4S_MASKED_SPLIT_FLOP", SPLIT_FLOP, 1, (1 << 63) - 1),
            "lds_small": _env(env, "G4S_MASKED_LDS_SMALL", LDS_SMALL, 0, LDS_SMALL),
            "lds_large": _env(env, "G4S_MASKED_LDS_LARGE", LDS_LARGE, 0, LDS_LARGE),
            "split_ways": _env(env, "G4S_MASKED_SPLIT_WAYS", SPLIT_WAYS, 2, 4096)}


def row_class(mlen, flop, cuts):
    """The class of a row whose mask row has `mlen` entries and which has `flop` products, from the documented rule (include/g4s.h, the header of
    spgemm_masked.hip): nothing asked for or nothing to look up — skip (the value stays at the identity). A row of more products than the split threshold is
    divided over several workgroups, each with an LDS table of its own when the mask row fits the small table, else searching the mask row in HBM. Otherwise a
    mask row of at most 64 entries with at most the wave class's products runs on one wavefront; a mask row that fits the small table, then the large table, is
    a table in LDS; a longer one is the global class."""
    if mlen == 0 or flop == 0:
        return "skip"
    fits_small, fits_large = mlen <= cuts["lds_small"], mlen <= cuts["lds_large"]
    if flop > cuts["split_flop"]:
        return "split_lds" if fits_small else "split_global"
    if mlen <= cuts["wave_mask"] and flop <= cuts["wave_flop"]:
        return "wave"
    return "lds_small" if fits_small else "lds_large" if fits_large else "global"


def counts_of(mlens, flops, cuts):
    """The seven class counts and the product sum of rows given by their mask lengths and product counts: the numbers of the library's debug line."""
    out = dict.fromkeys(CLASSES, 0)
    products = 0
    for mlen, flop in zip(mlens, flops):
        c = row_class(int(mlen), int(flop), cuts)
        out[c] += 1
        if c != "skip":
            products += int(flop)                                      # `atomicAdd(&s_prod, (unsigned long long)flop);` only for rows with work
    out["products"] = products
    return out


def info_of(counts):
    """The four merged fields of g4s_masked_info: `rows_lds = C_LDS_S + C_LDS_L + C_SPLIT_LDS`, `rows_global = C_GLOBAL + C_SPLIT_GLOBAL`,
    `rows_split = C_SPLIT_LDS + C_SPLIT_GLOBAL`."""
    return {"rows_wave": counts["wave"], "rows_lds": counts["lds_small"] + counts["lds_large"] + counts["split_lds"],
            "rows_global": counts["global"] + counts["split_global"], "rows_split": counts["split_lds"] + counts["split_global"]}


def debug_line(counts):
    """the line as the library formats it"""
    return ("g4s masked classes: skip %d wave %d lds_small %d lds_large %d global %d split_lds %d split_global %d (products %d)"
            % tuple(counts[k] for k in CLASSES + ("products",)))


class Row(NamedTuple):
    tag: str
    mlen: int                # entries of the mask row
    na: int                  # entries of the A row
    flop: int                # products: Σ over the A row's entries of the length of the B row
    cls: tuple               # ((mode, class), …) for every mode the case runs, from row_class
    declared: tuple          # ((mode, class), …) written by hand at the builder: the CPU test holds them against the model
    hits: str                # "both": the mask row must hold hits and identities; "all" / "none"; "" for no claim


class Edge(NamedTuple):
    const: str               # the cut the pair stands on: a key of cuts_of()
    mode: str                # the mode in which the pair straddles it
    at: str                  # tag of the row at the cut
    past: str                # tag of the row one past it
    at_cls: str
    past_cls: str


class Case(NamedTuple):
    name: str
    A: tuple                 # (rowptr int32, colids int32, values float64)
    B: tuple
    mask: tuple              # (mrpt int32, mcol int32)
    M: int
    K: int
    N: int
    rows: tuple              # Row per row of A
    edges: tuple
    semirings: tuple


def cls_of(row, mode):
    return dict(row.cls)[mode]


# ------------------------------------------------------------------------------------------------ builders
class _Build:
    """B rows with prescribed lengths (so that an A row reaches a prescribed product count exactly) and prescribed columns (so that a product lands below, on
    or above a mask column); A rows as lists of B rows IN THE ORDER GIVEN (the tiles of A entries are part of what is tested), each with its mask row."""

    def __init__(self, N, seed):
        self.N, self.rng = N, np.random.default_rng(seed)
        self.brows, self.arows, self.mrows, self.rows, self.bval, self.aval = [], [], [], [], {}, {}

    def brow(self, cols):
        cols = np.unique(np.asarray(cols, np.int64))
        assert cols.size == 0 or (cols[0] >= 0 and cols[-1] < self.N)
        self.brows.append(cols)
        return len(self.brows) - 1

    def empty(self):
        return self.brow([])

    def random_brow(self, n, lo=0, hi=None, have=()):
        """n distinct columns of [lo, hi), those of `have` among them"""
        hi = self.N if hi is None else hi
        pool = np.setdiff1d(np.arange(lo, hi), np.asarray(have, np.int64))
        return self.brow(np.concatenate([self.rng.choice(pool, n - len(have), replace=False), np.asarray(have, np.int64)]))

    def exact(self, flop, na, lo=0, hi=None):
        """na fresh B rows whose lengths add up to flop exactly (the first flop % na one longer than the rest; rows of length 0 where flop < na)"""
        base, rem = divmod(flop, na)
        return [self.random_brow(base + (i < rem), lo, hi) for i in range(na)]

    def mask(self, n, lo=0, hi=None, have=()):
        hi = self.N if hi is None else hi
        pool = np.setdiff1d(np.arange(lo, hi), np.asarray(have, np.int64))
        return np.sort(np.concatenate([self.rng.choice(pool, n - len(have), replace=False), np.asarray(have, np.int64)]))

    def set_b(self, b, col, value):
        self.bval[(b, int(np.searchsorted(self.brows[b], col)))] = float(value)

    def row(self, tag, brows, mask, mlen, flop, declared=None, hits="", avals=None):
        mask = np.asarray(mask, np.int64)
        assert mask.size == 0 or (np.all(np.diff(mask) > 0) and mask[0] >= 0 and mask[-1] < self.N)
        for pos, v in (avals or {}).items():
            self.aval[(len(self.arows), pos)] = float(v)
        self.arows.append(np.asarray(brows, np.int64))
        self.mrows.append(mask)
        declared = {"default": declared} if isinstance(declared, str) else (declared or {})
        self.rows.append(Row(tag, int(mlen), len(brows), int(flop), (), tuple(declared.items()), hits))

    def flop_of(self, brows):
        return int(sum(len(self.brows[b]) for b in brows))

    def ordinary(self, n=5, mlen=12):
        """a few ordinary rows around the edges: two to four B rows that exist already and a short mask row drawn from their columns and from the others"""
        short = [b for b, r in enumerate(self.brows) if 0 < len(r) <= 400]
        for i in range(n):
            pick = [int(x) for x in self.rng.choice(short, size=min(len(short), int(self.rng.integers(2, 5))), replace=False)]
            own = np.unique(np.concatenate([self.brows[b] for b in pick]))
            cols = np.unique(np.concatenate([self.rng.choice(own, min(own.size, mlen // 2), replace=False), self.rng.integers(0, self.N, mlen // 2)]))
            self.row(f"ordinary_{i}", pick, cols, cols.size, self.flop_of(pick))

    def skips(self):
        """the three ways to be skipped: something asked for and no entry of A; only empty rows of B; products and nothing asked for"""
        some = next(b for b, r in enumerate(self.brows) if len(r) > 0)
        self.row("skip_na_0", [], self.mask(5), 5, 0, "skip", "none")
        self.row("skip_only_empty_b_rows", [self.empty(), self.empty(), self.empty()], self.mask(7), 7, 0, "skip", "none")
        self.row("skip_no_mask", [some], [], 0, len(self.brows[some]), "skip")

    def finish(self, name, edges=(), semirings=SEMIRINGS):
        rng = self.rng
        K, M = len(self.brows), len(self.arows)
        ints = lambda n: rng.integers(-4, 5, n).astype(np.float64)
        rp = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        cat = lambda rows: (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
        brp, bci, arp, aci, mrp, mci = rp(self.brows), cat(self.brows), rp(self.arows), cat(self.arows), rp(self.mrows), cat(self.mrows)
        ava, bva = ints(aci.size), ints(bci.size)
        few = np.repeat(np.diff(arp) < 8, np.diff(arp)) & (ava == 0)    # a zero in a row of a few entries would zero the whole row: those rows keep no zeros
        ava[few] = rng.choice([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0], int(few.sum()))
        for (i, pos), v in self.aval.items():
            ava[arp[i] + pos] = v
        for (b, pos), v in self.bval.items():
            bva[brp[b] + pos] = v
        A, B, mask = (arp, aci, ava), (brp, bci, bva), (mrp, mci)
        for a in A + B + mask:
            a.setflags(write=False)
        tags = [r.tag for r in self.rows]
        assert len(set(tags)) == len(tags)
        modes = RUNS[name]
        rows = tuple(r._replace(cls=tuple((m, row_class(r.mlen, r.flop, cuts_of(MODES[m]))) for m in modes)) for r in self.rows)
        return Case(name, A, B, mask, M, K, self.N, rows, tuple(edges), tuple(semirings))


def _grid():
    """(mask length, products) ∈ {1, 63, 64, 65} × {1, 4095, 4096, 4097}: (64, 4096) is the last wave row; (65, ·) and (·, 4097) take the small LDS table.
    mlen = 1 with 4 097 products is the LDS class with a table of one entry (cmin = cmax)."""
    b = _Build(700, 101)
    u1, u2 = b.brow([100]), b.brow([101])
    r273 = [b.random_brow(273, 0, 500, have=[100] if i % 5 == 0 else []) for i in range(15)]   # 15 · 273 = 4 095, on the columns below 500: a mask column above gets nothing
    by_flop = {1: [u1], 4095: r273, 4096: r273 + [u1], 4097: r273 + [u1, u2]}
    edges = []
    for mlen in (1, 63, 64, 65):
        for flop, brows in by_flop.items():
            cls = "wave" if mlen <= 64 and flop <= 4096 else "lds_small"
            b.row(f"m{mlen}_f{flop}", brows, b.mask(mlen, have=[100]), mlen, flop, {"default": cls, "lds_over": cls, "lds_small_0": "wave" if cls == "wave" else "lds_large"},
                  "both" if mlen > 1 else "all")
        if mlen <= 64:
            edges += [Edge("wave_flop", m, f"m{mlen}_f4096", f"m{mlen}_f4097", "wave", "lds_small") for m in ("default", "lds_over")]
            edges.append(Edge("wave_flop", "lds_small_0", f"m{mlen}_f4096", f"m{mlen}_f4097", "wave", "lds_large"))
    for flop in (1, 4095, 4096):
        edges.append(Edge("wave_mask", "default", f"m64_f{flop}", f"m65_f{flop}", "wave", "lds_small"))
    b.skips()
    b.ordinary()
    return b.finish("grid", edges)


def _wave_tiles():
    """The wave kernel's own edges: tiles of 64 entries of A (a second tile, a last tile of one entry), empty rows of B at the start, in the middle and at the
    end of a tile, a whole tile of empty rows, tiles of 64, 65 and 128 products (the e0 loop), products below and above every mask column (with fewer than 64
    mask entries the search ends on an INT_MAX pad, with 64 on the last column), on the first and the last mask column, and column N − 1."""
    N = 200
    b = _Build(N, 102)
    single = [b.brow([10 + i % 90]) for i in range(129)]               # columns 10 … 99, each of the first 39 twice
    empties = [b.empty() for _ in range(64)]
    even = lambda n: 10 + 2 * np.arange(n)                             # the mask row 10, 12, …: the singles on odd columns miss, those above 8 + 2n lie above it
    for na in (1, 63, 64, 65, 128, 129):
        b.row(f"na_{na}", single[:na], np.concatenate([even(40), [110, 120]]), 42, na, "wave", "both" if na > 1 else "")   # (no single reaches 110 or 120)
    gaps = list(single[:64])
    gaps[0], gaps[31], gaps[63] = empties[0], empties[1], empties[2]
    b.row("empty_b_first_mid_last_of_tile", gaps, even(40), 40, 61, "wave", "both")
    b.row("tile_0_all_empty", empties + single[:64], even(40), 40, 64, "wave", "both")
    b.row("tile_1_all_empty", single[:64] + empties, even(40), 40, 64, "wave", "both")
    b.row("tile_1_of_3_all_empty", single[:64] + empties + single[64:66], even(40), 40, 66, "wave", "both")
    b64, b64b, b1 = b.brow(np.arange(10, 74)), b.brow(np.arange(40, 104)), b.brow([12])
    b.row("tile_total_64", [b64], even(50), 50, 64, "wave", "both")
    b.row("tile_total_65", [b64, b1], even(50), 50, 65, "wave", "both")
    b.row("tile_total_128", [b64, b64b], even(50), 50, 128, "wave", "both")
    b.row("tile_total_129", [b64, b1, b64b], even(50), 50, 129, "wave", "both")
    below, above = b.brow([1, 4, 7, 9]), b.brow([140, 150, 199])
    b.row("all_below_the_mask", [below], even(40), 40, 4, "wave", "none")
    b.row("all_above_the_mask_pad", [above], even(40), 40, 3, "wave", "none")            # 40 < 64: the lower bound ends on an INT_MAX pad
    b.row("all_above_the_mask_63", [above], even(63), 63, 3, "wave", "none")              # one pad
    b.row("all_above_the_mask_64", [above], even(64), 64, 3, "wave", "none")              # no pad: the lower bound ends on the last column, 136
    b.row("below_and_above_and_hits", [below, above, b1], even(40), 40, 8, "wave", "both")
    for mlen in (63, 64):
        ends = b.brow([10, 8 + 2 * mlen])
        b.row(f"first_and_last_column_m{mlen}", [ends], even(mlen), mlen, 2, "wave", "both")
    last = b.brow([150, N - 1])
    b.row("column_n_minus_1", [last, b1], np.concatenate([even(20), [N - 1]]), 21, 3, "wave", "both")
    b.row("column_n_minus_1_m64", [last, b1], np.concatenate([even(63), [N - 1]]), 64, 3, "wave", "both")
    b.skips()
    return b.finish("wave_tiles")


def _wave_rows(n):
    """exactly n rows of the wave class (and the skipped ones): with four rows per workgroup the last workgroup holds n % 4 of them"""
    b = _Build(120, 110 + n)
    pool = [b.random_brow(int(k)) for k in b.rng.integers(1, 30, 12)]
    b.skips()
    for i in range(n):
        pick = [int(x) for x in b.rng.choice(len(pool), 3, replace=False)]
        own = np.unique(np.concatenate([b.brows[pool[p]] for p in pick]))
        cols = np.unique(np.concatenate([own[::3], np.setdiff1d(np.arange(120), own)[i::9]]))
        b.row(f"wave_{i}", [pool[p] for p in pick], cols, cols.size, b.flop_of([pool[p] for p in pick]), "wave", "both")
    return b.finish(f"wave_rows_{n}")


def _row256():
    """The 256-thread row kernel (small LDS table): A rows of 255, 256, 257, 512 and 513 entries (tiles of 256), products on cmin − 1, cmin, cmax and cmax + 1,
    a table of one entry reached by its products, the table exactly full at 1 024 entries and the row of 1 025 that takes the large table."""
    N = 3000
    b = _Build(N, 103)
    pool = [b.random_brow(i % 3, 500, 900) for i in range(513)]        # lengths 0, 1, 2, …: empty rows of B all along the tiles
    wide = b.mask(100, 500, 900)
    for na in (255, 256, 257, 512, 513):
        b.row(f"na_{na}", pool[:na], wide, 100, b.flop_of(pool[:na]), "lds_small", "both")
    clip = 1000 + 2 * np.arange(80)                                    # cmin = 1000, cmax = 1158
    b.row("clip_edges", [b.brow([999, 1000, 1158, 1159])], clip, 80, 4, "lds_small", "both")
    b.row("clip_below", [b.brow([998, 999])], clip, 80, 2, "lds_small", "none")
    b.row("clip_above", [b.brow([1159, 2999])], clip, 80, 2, "lds_small", "none")
    r1000 = [b.random_brow(1000, 0, 2990, have=[1500] if i < 3 else []) for i in range(5)]
    b.row("mlen_1_flop_5000", r1000, [1500], 1, 5000, "lds_small", "all")
    b.row("mlen_1_flop_5000_miss", r1000, [2995], 1, 5000, "lds_small", "none")
    b.row("mlen_1024", r1000, b.mask(1024, have=[0, N - 1]), 1024, 5000, {"default": "lds_small", "lds_large_0": "lds_small", "lds_small_0": "lds_large"}, "both")
    b.row("mlen_1025", r1000, b.mask(1025, have=[0, N - 1]), 1025, 5000, {"default": "lds_large", "lds_large_0": "global", "lds_over": "lds_large"}, "both")
    b.row("mlen_1024_few_products", pool[:9], b.mask(1024, 400, 1500), 1024, b.flop_of(pool[:9]), "lds_small", "both")
    b.skips()
    b.ordinary()
    edges = [Edge("lds_small", m, "mlen_1024", "mlen_1025", "lds_small", "lds_large") for m in ("default", "lds_over")]
    return b.finish("row256", edges)


def _row1024():
    """The 1 024-thread row kernel (large LDS table): A rows of 1 023, 1 024, 1 025 and 2 049 entries, the table exactly full at 8 192 entries — once with a
    product in every slot — and the rows of 8 193 entries and of N entries (a full-width mask row) that take the global class."""
    N = 8300
    b = _Build(N, 104)
    pool = [b.random_brow(i % 3) for i in range(2049)]
    wide = b.mask(2000)
    for na in (1023, 1024, 1025, 2049):
        b.row(f"na_{na}", pool[:na], wide, 2000, b.flop_of(pool[:na]), "lds_large", "both")
    full = 50 + np.arange(8192)
    lo, hi, alt = b.brow(full[:4096]), b.brow(full[4096:]), b.brow(full[::2])
    moved = {"lds_large_2000": "global", "lds_large_0": "global", "lds_small_0": "lds_large", "lds_over": "lds_large"}
    b.row("mlen_8192_every_slot", [lo, hi, alt], full, 8192, 12288, {"default": "lds_large", **moved}, "all")
    r3000 = [b.random_brow(3000) for _ in range(3)]
    b.row("mlen_8192", r3000, b.mask(8192, have=[0, N - 1]), 8192, 9000, {"default": "lds_large", **moved}, "both")
    b.row("mlen_8193", r3000, b.mask(8193, have=[0, N - 1]), 8193, 9000, {"default": "global", "lds_over": "global"}, "both")
    b.row("mlen_n", r3000[:2], np.arange(N), N, 6000, "global", "both")
    b.row("mlen_1025", pool[:40], b.mask(1025), 1025, b.flop_of(pool[:40]), {"default": "lds_large", "lds_large_0": "global"})
    b.skips()
    b.ordinary()
    edges = [Edge("lds_large", m, "mlen_8192", "mlen_8193", "lds_large", "global") for m in ("default", "lds_over")]
    return b.finish("row1024", edges)


def _split(mlen):
    """2^20 products against 2^20 + 1 in rows of 1 024 entries of A — four tiles of 256, fewer than the 128 parts: parts 0 … 3 work, part 4 starts exactly at the
    row's end and returns with the 123 behind it. mlen = 1 024: the small LDS table against the split row that folds 4 private tables into cval; mlen = 1 025:
    the large table against the split row that searches the mask row in HBM. Two mask columns receive +k and −k and nothing else: 3001 from two entries of the
    first tile (the sum is 0.0 inside one table; the fold skips it as an identity), 3002 from the first and the last tile (two parts add +4 and −4 to cval).
    The mask columns above 3100 receive nothing."""
    N = 4200
    b = _Build(N, 105 + mlen % 2)
    z1, z2 = 3001, 3002
    p, q = b.random_brow(1024, 0, 3003, have=[z1, z2]), b.random_brow(1024, 0, 3001)
    b.brows[q] = np.unique(np.concatenate([b.brows[q][:-1], [z1]]))    # 1 023 columns below 3001 and z1
    body = [b.random_brow(1024, 0, 3000) for _ in range(1021)]
    longer = b.random_brow(1025, 0, 3000)
    s = b.brow(np.concatenate([b.brows[body[0]][:-1], [z2]]))
    assert all(len(b.brows[x]) == 1024 for x in (p, q, s))
    for brow, col, v in ((p, z1, 3), (q, z1, -3), (p, z2, 2), (s, z2, -2)):
        b.set_b(brow, col, v)
    mask = np.sort(np.concatenate([b.rng.choice(3000, 900, replace=False), [z1, z2], 3100 + b.rng.choice(N - 3100, mlen - 902, replace=False)]))
    two = {0: 2, 1: 2, 1023: 2}                                        # A's values on p, q and s
    small = mlen <= LDS_SMALL
    b.row("flop_2p20", [p, q] + body + [s], mask, mlen, 1 << 20, "lds_small" if small else "lds_large", "both", avals=two)
    b.row("flop_2p20_plus_1", [p, q] + body[:-1] + [longer, s], mask, mlen, (1 << 20) + 1, "split_lds" if small else "split_global", "both", avals=two)
    b.row("small_row", [body[3]], mask[::40], len(mask[::40]), 1024, "wave", "both")
    b.skips()
    edges = [Edge("split_flop", "default", "flop_2p20", "flop_2p20_plus_1", *(("lds_small", "split_lds") if small else ("lds_large", "split_global")))]
    return b.finish(f"split_mlen_{mlen}", edges, semirings=SEMIRINGS[:2])


def _moved():
    """Every cut moved down by its environment variable, with a row at the moved cut and one past it; under split_flop_20000 all seven classes occur at once.
    The rows of more than 20 000 products have 2·256, 2·256 + 1, 3·256 and 3·256 + 1 entries of A: with 2 and 3 parts that is a second round of
    `a0 += ways·TPB` for every part, for the first part only, or for none."""
    N = 8300
    b = _Build(N, 107)
    m10, m100, m101, m2000, m2001 = b.mask(10), b.mask(100), b.mask(101), b.mask(2000), b.mask(2001)
    m1024, m1025, m8193 = b.mask(1024), b.mask(1025), b.mask(8193)
    m10_out = np.concatenate([b.mask(7, 0, 8000), [8100, 8200, N - 1]])          # three columns that no product reaches
    f100 = b.exact(100, 7, 0, 400)
    split = ("split_flop_20000", "split_ways_2", "split_ways_3")
    b.row("flop_100", f100, m10, 10, 100, {"default": "wave", "wave_flop_100": "wave"}, "")
    b.row("flop_101", f100 + [b.brow([m10[0]])], m10, 10, 101, {"default": "wave", "wave_flop_100": "lds_small"}, "both")
    f300 = b.exact(300, 20)
    b.row("mlen_100", f300, m100, 100, 300, {"default": "lds_small", "lds_small_100": "lds_small", "lds_small_0": "lds_large", "lds_large_0": "lds_small"})
    b.row("mlen_101", f300, m101, 101, 300, {"default": "lds_small", "lds_small_100": "lds_large"})
    b.row("mlen_2000", f300, m2000, 2000, 300, {"default": "lds_large", "lds_large_2000": "lds_large", "lds_large_0": "global"}, "both")
    b.row("mlen_2001", f300, m2001, 2001, 300, {"default": "lds_large", "lds_large_2000": "global"}, "both")
    b.row("mlen_8193", f300, m8193, 8193, 300, {"default": "global", "lds_small_0": "global", "lds_over": "global"}, "both")
    at, past = b.exact(20000, 512, 0, 8000), b.exact(20001, 513, 0, 8000)
    b.row("flop_20000_na_512", at, m100, 100, 20000, {"default": "lds_small", **dict.fromkeys(split, "lds_small")}, "both")
    b.row("flop_20001_na_513", past, m100, 100, 20001, {"default": "lds_small", **dict.fromkeys(split, "split_lds")}, "both")
    b.row("flop_20001_na_512_m1024", b.exact(20001, 512, 0, 8000), m1024, 1024, 20001, {"default": "lds_small", **dict.fromkeys(split, "split_lds")}, "both")
    b.row("flop_20000_na_513_m1025", b.exact(20000, 513, 0, 8000), m1025, 1025, 20000, {"default": "lds_large", **dict.fromkeys(split, "lds_large")}, "both")
    b.row("flop_20001_na_768_m1025", b.exact(20001, 768, 0, 8000), m1025, 1025, 20001, {"default": "lds_large", **dict.fromkeys(split, "split_global")}, "both")
    b.row("flop_20001_na_769_m1024", b.exact(20001, 769, 0, 8000), m1024, 1024, 20001, {"default": "lds_small", **dict.fromkeys(split, "split_lds")}, "both")
    b.row("flop_40000_na_769_m8193", b.exact(40000, 769, 0, 8000), m8193, 8193, 40000, {"default": "global", **dict.fromkeys(split, "split_global")}, "both")
    b.row("flop_30000_na_768_m10", b.exact(30000, 768, 0, 8000), m10_out, 10, 30000, {"default": "lds_small", **dict.fromkeys(split, "split_lds")}, "both")
    b.skips()
    b.ordinary()
    edges = [Edge("wave_flop", "wave_flop_100", "flop_100", "flop_101", "wave", "lds_small"),
             Edge("lds_small", "lds_small_100", "mlen_100", "mlen_101", "lds_small", "lds_large"),
             Edge("lds_large", "lds_large_2000", "mlen_2000", "mlen_2001", "lds_large", "global")]
    for m in split:
        edges += [Edge("split_flop", m, "flop_20000_na_512", "flop_20001_na_513", "lds_small", "split_lds"),
                  Edge("split_flop", m, "flop_20000_na_513_m1025", "flop_20001_na_768_m1025", "lds_large", "split_global"),
                  Edge("lds_small", m, "flop_20001_na_512_m1024", "flop_20001_na_768_m1025", "split_lds", "split_global")]
    return b.finish("moved", edges)


_ONLY = {"lds_small": (100, "default"), "lds_large": (1500, "default"), "global": (8193, "default"), "split_lds": (100, "split_flop_20000"),
         "split_global": (8193, "split_flop_20000")}


def _only(cls):
    """Three rows of one class and the skipped rows: six of the seven class lists are empty (the wave class: wave_rows_*)."""
    mlen, mode = _ONLY[cls]
    b = _Build(8300, 120 + CLASSES.index(cls))
    for i in range(3):
        flop, na = (20001 + 500 * i, 300 + 256 * i) if cls.startswith("split") else (4097 + i, 30 + i)
        b.row(f"{cls}_{i}", b.exact(flop, na), b.mask(mlen + (i if mlen < 8000 else 0)), mlen + (i if mlen < 8000 else 0), flop, {mode: cls}, "both")
    b.skips()
    return b.finish(f"only_{cls}")


def _wave_and_global():
    """classes missing in the middle: only the wave and the global list (and the skipped rows) — off[] skips three empty lists"""
    b = _Build(8300, 130)
    pool = b.exact(200, 9)
    for i in range(3):
        b.row(f"wave_{i}", pool[i:i + 4], b.mask(10 + i), 10 + i, b.flop_of(pool[i:i + 4]), "wave")
    b.skips()
    for i in range(2):
        b.row(f"global_{i}", pool[i:i + 6], b.mask(8193 + i), 8193 + i, b.flop_of(pool[i:i + 6]), "global", "both")
    return b.finish("wave_and_global")


def _open(M):
    """The opening pass: M rows (32 per workgroup), mask rows of 0 to 9 entries — fewer, as many and more than the 8 lanes of a row — each drawn anew from all
    columns, so that a row starts below the last column of the row before it."""
    b = _Build(40, 140 + M)
    pool = [b.random_brow(int(k)) for k in b.rng.integers(0, 6, 10)]
    for i in range(M):
        mlen = (i + 3) % 10
        pick = [pool[int(x)] for x in b.rng.choice(len(pool), int(b.rng.integers(0, 4)), replace=False)]
        b.row(f"row_{i}_mlen_{mlen}", pick, b.mask(mlen), mlen, b.flop_of(pick), "wave" if mlen and b.flop_of(pick) else "skip")
    return b.finish(f"open_{M}")


_BUILDERS = {
    "grid": _grid, "wave_tiles": _wave_tiles, "row256": _row256, "row1024": _row1024,
    "split_mlen_1024": functools.partial(_split, 1024), "split_mlen_1025": functools.partial(_split, 1025), "moved": _moved,
    **{f"wave_rows_{n}": functools.partial(_wave_rows, n) for n in (1, 3, 4, 5)},
    **{f"only_{c}": functools.partial(_only, c) for c in _ONLY},
    "wave_and_global": _wave_and_global,
    **{f"open_{M}": functools.partial(_open, M) for M in (1, 31, 32, 33)},
}
NAMES = list(_BUILDERS)
BIG = ("split_mlen_1024", "split_mlen_1025")     # two million products: plus-times and min-plus only

# Each case with the modes that move its rows.
RUNS = {
    "grid": ("default", "lds_small_0", "lds_over"),
    "wave_tiles": ("default", "wave_flop_100"),
    "row256": ("default", "lds_small_0", "lds_large_0", "lds_over"),
    "row1024": ("default", "lds_large_2000", "lds_small_0", "lds_large_0", "lds_over"),
    "split_mlen_1024": ("default",),
    "split_mlen_1025": ("default",),
    "moved": tuple(MODES),
    **{f"wave_rows_{n}": ("default",) for n in (1, 3, 4, 5)},
    "only_lds_small": ("default",), "only_lds_large": ("default",), "only_global": ("default",),
    "only_split_lds": ("default", "split_flop_20000", "split_ways_3"), "only_split_global": ("default", "split_flop_20000", "split_ways_2"),
    "wave_and_global": ("default", "split_flop_20000"),
    **{f"open_{M}": ("default",) for M in (1, 31, 32, 33)},
}
HOST_FORM = ("wave_rows_5", "only_lds_small", "only_lds_large", "only_global", "only_split_lds", "only_split_global")   # one case per class, host pointers


def semirings_of(name):
    """the semirings the GPU test runs the case over (known without building it)"""
    return SEMIRINGS[:2] if name in BIG else SEMIRINGS


@functools.lru_cache(maxsize=None)
def build(name):
    """The case (cached: its arrays are read-only)."""
    return _BUILDERS[name]()


def row(case, tag):
    return next(r for r in case.rows if r.tag == tag)


def operands(case, semiring):
    """A and B as the GPU test multiplies them: or-and gets further stored zeros (a fifth of the entries exist with the value 0.0), as in the semiring tests"""
    if semiring != "or_and":
        return case.A, case.B
    rng = np.random.default_rng(7)
    out = []
    for rp, ci, va in (case.A, case.B):
        v = va.copy()
        v[rng.random(v.size) < 0.2] = 0.0
        v.setflags(write=False)
        out.append((rp, ci, v))
    return tuple(out)


def expected_counts(case, mode, cuts=None):
    """The seven counts and the product sum that the `g4s masked classes:` line must show (cuts: the model with a number moved, for the sensitivity check)."""
    return counts_of([r.mlen for r in case.rows], [r.flop for r in case.rows], cuts or cuts_of(MODES[mode]))


def expected_info(case, mode):
    return info_of(expected_counts(case, mode))


# ------------------------------------------------------------------------------------------------ every edge against the rows that stand on it
# edge: [(case, row tag, mode, {field of the Row, or "cls": its class in that mode}), …] — checked by tests/test_masked_cases_cpu.py
def _c(case, tag, mode="default", **want):
    return case, tag, mode, want


COVERAGE = {
    # class cuts, default environment
    **{f"grid_m{m}_f{f}": [_c("grid", f"m{m}_f{f}", mlen=m, flop=f, cls="wave" if m <= 64 and f <= 4096 else "lds_small")]
       for m in (1, 63, 64, 65) for f in (1, 4095, 4096, 4097)},
    "mlen_1024_with_1025": [_c("row256", "mlen_1024", mlen=1024, cls="lds_small"), _c("row256", "mlen_1025", mlen=1025, cls="lds_large")],
    "mlen_8192_with_8193": [_c("row1024", "mlen_8192", mlen=8192, cls="lds_large"), _c("row1024", "mlen_8193", mlen=8193, cls="global")],
    "flop_2p20_small_mask": [_c("split_mlen_1024", "flop_2p20", flop=1 << 20, cls="lds_small"),
                             _c("split_mlen_1024", "flop_2p20_plus_1", flop=(1 << 20) + 1, cls="split_lds")],
    "flop_2p20_mlen_1025": [_c("split_mlen_1025", "flop_2p20", mlen=1025, flop=1 << 20, cls="lds_large"),
                            _c("split_mlen_1025", "flop_2p20_plus_1", mlen=1025, flop=(1 << 20) + 1, cls="split_global")],
    "split_row_mlen_1024_with_1025": [_c("split_mlen_1024", "flop_2p20_plus_1", mlen=1024, cls="split_lds"),
                                      _c("split_mlen_1025", "flop_2p20_plus_1", mlen=1025, cls="split_global"),
                                      _c("moved", "flop_20001_na_512_m1024", "split_flop_20000", mlen=1024, cls="split_lds"),
                                      _c("moved", "flop_20001_na_768_m1025", "split_flop_20000", mlen=1025, cls="split_global")],
    "skip_mask_without_products": [_c("grid", "skip_na_0", flop=0, cls="skip"), _c("grid", "skip_only_empty_b_rows", flop=0, na=3, cls="skip")],
    "skip_products_without_mask": [_c("grid", "skip_no_mask", mlen=0, cls="skip")],
    # the same cuts moved by the environment
    "env_wave_flop_100": [_c("moved", "flop_100", "wave_flop_100", flop=100, cls="wave"), _c("moved", "flop_101", "wave_flop_100", flop=101, cls="lds_small")],
    "env_lds_small_100": [_c("moved", "mlen_100", "lds_small_100", mlen=100, cls="lds_small"), _c("moved", "mlen_101", "lds_small_100", mlen=101, cls="lds_large")],
    "env_lds_large_2000": [_c("moved", "mlen_2000", "lds_large_2000", mlen=2000, cls="lds_large"), _c("moved", "mlen_2001", "lds_large_2000", mlen=2001, cls="global")],
    "env_split_flop_20000": [_c("moved", "flop_20000_na_512", "split_flop_20000", flop=20000, cls="lds_small"),
                             _c("moved", "flop_20001_na_513", "split_flop_20000", flop=20001, cls="split_lds"),
                             _c("moved", "flop_20000_na_513_m1025", "split_flop_20000", flop=20000, cls="lds_large"),
                             _c("moved", "flop_20001_na_768_m1025", "split_flop_20000", flop=20001, cls="split_global")],
    "env_split_ways_2": [_c("moved", t, "split_ways_2", na=na) for t, na in (("flop_20001_na_512_m1024", 512), ("flop_20001_na_513", 513),
                                                                          ("flop_20001_na_768_m1025", 768), ("flop_20001_na_769_m1024", 769))],
    "env_split_ways_3": [_c("moved", t, "split_ways_3", na=na) for t, na in (("flop_20001_na_512_m1024", 512), ("flop_20001_na_513", 513),
                                                                          ("flop_20001_na_768_m1025", 768), ("flop_20001_na_769_m1024", 769))],
    "env_lds_small_0": [_c("moved", "mlen_100", "lds_small_0", cls="lds_large"), _c("row256", "mlen_1024", "lds_small_0", cls="lds_large"),
                        _c("grid", "m65_f1", "lds_small_0", cls="lds_large"), _c("grid", "m64_f4096", "lds_small_0", cls="wave")],
    "env_lds_large_0": [_c("moved", "mlen_2000", "lds_large_0", cls="global"), _c("row256", "mlen_1025", "lds_large_0", cls="global"),
                        _c("row256", "mlen_1024", "lds_large_0", cls="lds_small")],
    "env_clamp_above_range": [_c("row256", "mlen_1025", "lds_over", cls="lds_large"), _c("row1024", "mlen_8193", "lds_over", cls="global"),
                              _c("row1024", "mlen_8192", "lds_over", cls="lds_large"), _c("row256", "mlen_1024", "lds_over", cls="lds_small")],
    # wave kernel
    **{f"wave_na_{na}": [_c("wave_tiles", f"na_{na}", na=na, cls="wave")] for na in (1, 63, 64, 65, 128, 129)},
    "wave_empty_b_rows_in_tile": [_c("wave_tiles", "empty_b_first_mid_last_of_tile", na=64, flop=61, cls="wave")],
    "wave_tile_all_empty": [_c("wave_tiles", "tile_0_all_empty", na=128, cls="wave"), _c("wave_tiles", "tile_1_all_empty", na=128, cls="wave"),
                            _c("wave_tiles", "tile_1_of_3_all_empty", na=130, cls="wave")],
    "wave_tile_total_64_65_128": [_c("wave_tiles", f"tile_total_{f}", flop=f, cls="wave") for f in (64, 65, 128, 129)],
    "wave_below_every_mask_column": [_c("wave_tiles", "all_below_the_mask", cls="wave")],
    "wave_above_every_mask_column": [_c("wave_tiles", "all_above_the_mask_pad", mlen=40, cls="wave"), _c("wave_tiles", "all_above_the_mask_63", mlen=63, cls="wave"),
                                     _c("wave_tiles", "all_above_the_mask_64", mlen=64, cls="wave")],
    "wave_first_and_last_mask_column": [_c("wave_tiles", "first_and_last_column_m63", mlen=63, cls="wave"), _c("wave_tiles", "first_and_last_column_m64", mlen=64, cls="wave")],
    "wave_column_n_minus_1": [_c("wave_tiles", "column_n_minus_1", cls="wave"), _c("wave_tiles", "column_n_minus_1_m64", mlen=64, cls="wave")],
    **{f"wave_rows_{n}": [_c(f"wave_rows_{n}", f"wave_{n - 1}", cls="wave")] for n in (1, 3, 4, 5)},
    # row kernel, 256 threads
    **{f"row256_na_{na}": [_c("row256", f"na_{na}", na=na, cls="lds_small")] for na in (255, 256, 257, 512, 513)},
    "row256_clip": [_c("row256", "clip_edges", flop=4, cls="lds_small"), _c("row256", "clip_below", cls="lds_small"), _c("row256", "clip_above", cls="lds_small")],
    "row256_mlen_1": [_c("row256", "mlen_1_flop_5000", mlen=1, flop=5000, cls="lds_small"), _c("grid", "m1_f4097", mlen=1, cls="lds_small")],
    "row256_table_full": [_c("row256", "mlen_1024", mlen=1024, cls="lds_small"), _c("row256", "mlen_1024_few_products", mlen=1024, cls="lds_small")],
    # row kernel, 1 024 threads
    **{f"row1024_na_{na}": [_c("row1024", f"na_{na}", na=na, cls="lds_large")] for na in (1023, 1024, 1025, 2049)},
    "row1024_table_full": [_c("row1024", "mlen_8192", mlen=8192, cls="lds_large")],
    "row1024_every_slot": [_c("row1024", "mlen_8192_every_slot", mlen=8192, hits="all", cls="lds_large")],
    # global class
    "global_mlen_8193": [_c("row1024", "mlen_8193", mlen=8193, cls="global")],
    "global_full_width": [_c("row1024", "mlen_n", mlen=8300, cls="global")],
    # split
    "split_tiles_fewer_than_ways": [_c("split_mlen_1024", "flop_2p20_plus_1", na=1024, cls="split_lds"), _c("split_mlen_1025", "flop_2p20_plus_1", na=1024, cls="split_global")],
    "split_ways_second_round": [_c("moved", "flop_20001_na_513", "split_ways_2", na=513, cls="split_lds"), _c("moved", "flop_20001_na_769_m1024", "split_ways_3", na=769, cls="split_lds"),
                                _c("moved", "flop_20001_na_768_m1025", "split_ways_2", na=768, cls="split_global"), _c("moved", "flop_40000_na_769_m8193", "split_ways_2", na=769, cls="split_global")],
    "split_sums_to_zero": [_c("split_mlen_1024", "flop_2p20_plus_1", cls="split_lds", hits="both")],
    "split_slots_without_products": [_c("split_mlen_1024", "flop_2p20_plus_1", hits="both"), _c("moved", "flop_30000_na_768_m10", "split_flop_20000", cls="split_lds", hits="both")],
    "split_three_rows_or_more": [_c("moved", "flop_20001_na_513", "split_flop_20000", cls="split_lds"), _c("only_split_lds", "split_lds_2", "split_flop_20000", cls="split_lds"),
                                 _c("only_split_global", "split_global_2", "split_flop_20000", cls="split_global")],
    # class lists
    **{f"only_{c}": [_c(f"only_{c}", f"{c}_0", mode, cls=c)] for c, (_, mode) in _ONLY.items()},
    "only_wave": [_c("wave_rows_3", "wave_0", cls="wave")],
    "all_seven_classes": [_c("moved", "flop_40000_na_769_m8193", "split_flop_20000", cls="split_global")],
    "only_wave_and_global": [_c("wave_and_global", "wave_0", cls="wave"), _c("wave_and_global", "global_1", cls="global")],
    # opening pass
    **{f"open_{M}": [_c(f"open_{M}", f"row_{M - 1}_mlen_{(M + 2) % 10}")] for M in (1, 31, 32, 33)},
}


# ------------------------------------------------------------------------------------------------ triangle counting: graphs and the model applied to L
def graph_csr(n, edges):
    """The symmetric simple graph of an edge list as (rowptr int32, colids int32), rows ascending."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    both = np.unique(np.concatenate([e, e[:, ::-1]]), axis=0) if e.size else e
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, both[:, 0] + 1, 1)
    return np.cumsum(rp).astype(np.int32), both[:, 1].astype(np.int32)


def lower_rows(rowptr, colids):
    """(mask length, products) of every row of L·L⟨L⟩, L the strictly lower triangle: the entries below the diagonal, and the sum of those counts over them."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    low = colids < rows
    mlen = np.bincount(rows[low], minlength=n).astype(np.int64)
    flop = np.zeros(n, np.int64)
    np.add.at(flop, rows[low], mlen[colids[low]])
    return mlen, flop


def clique(k):
    i, j = np.triu_indices(k, 1)
    return k, np.stack([i, j], 1)


def subset_with_sum(target, top):
    """distinct ids of [1, top] that add up to target, the largest first (top·(top + 1)/2 >= target)"""
    out, rest = [], target
    for v in range(top, 0, -1):
        if v <= rest:
            out.append(v)
            rest -= v
    assert rest == 0
    return out


def rows_with_products(flops=(4095, 4096, 4097), k=128):
    """A clique on the vertices 0 … k − 1 (vertex p has p lower neighbours) and one further vertex per entry of `flops`, joined to a set of clique vertices
    whose ids add up to that many products. Returns (n, edges, the ids of the further vertices)."""
    _, edges = clique(k)
    extra = []
    for t, flop in enumerate(flops):
        v = k + t
        extra.append(np.array([[v, p] for p in subset_with_sum(flop, k - 1)]))
    return k + len(flops), np.concatenate([edges] + extra), list(range(k, k + len(flops)))


def hub_over_ring(h, width=1):
    """The vertices 0 … h − 1 joined in a ring — each with the `width` vertices before it, cyclically — and the hub h joined to all of them: the hub's row of L
    has h entries and about width·h products. A plain ring (width 1) gives the hub h products and h triangles."""
    v = np.arange(h)
    ring = np.concatenate([np.stack([v, (v - d) % h], 1) for d in range(1, width + 1)])
    return h + 1, np.concatenate([ring, np.stack([np.full(h, h), v], 1)])
