"""g4s_color without a GPU: the numpy reference of tests/color_ref.py against networkx.greedy_color with the explicit order on every graph the GPU tests
use and under every order, the properties of a first-fit colouring, the property each new graph is named for; then the struct, constants and signature in
every layer, the exported symbol, argument refusals before any HIP call (G4S_ERR_INVALID), the C++ form of include/g4s/csr.hpp and examples/color.cpp
(compile only) and the Python ValueErrors."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import color_ref as ref
from tests import kcore_ref
from tests.test_cpp_host import _build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# (name, order) → (colours, rounds, overflow) of the reference
FACTS = {
    ("doubling_tree", "hash"): (42, 46, 0), ("doubling_tree", "largest_first"): (40, 47, 0), ("doubling_tree", "smallest_last"): (40, 55, 0),
    ("doubling_tree", "reverse_id"): (41, 55, 0), ("grid", "hash"): (5, 11, 0), ("grid", "largest_first"): (5, 11, 0), ("grid", "smallest_last"): (2, 82, 0),
    ("grid", "reverse_id"): (2, 127, 0), ("hub_leaves_clique", "hash"): (20, 20, 0), ("hub_leaves_clique", "largest_first"): (20, 21, 0),
    ("hub_leaves_clique", "smallest_last"): (20, 21, 0), ("hub_leaves_clique", "reverse_id"): (20, 21, 0), ("path", "hash"): (3, 6, 0),
    ("path", "largest_first"): (3, 6, 0), ("path", "smallest_last"): (2, 2001, 0), ("path", "reverse_id"): (2, 4001, 0), ("rmat13", "hash"): (60, 210, 0),
    ("rmat13", "largest_first"): (47, 197, 0), ("rmat13", "smallest_last"): (48, 233, 0), ("rmat13", "reverse_id"): (53, 167, 0), ("star", "hash"): (2, 2, 0),
    ("star", "largest_first"): (2, 2, 0), ("star", "smallest_last"): (2, 2, 0), ("star", "reverse_id"): (2, 2, 0), ("tiny", "hash"): (3, 3, 0),
    ("tiny", "largest_first"): (3, 3, 0), ("tiny", "smallest_last"): (3, 3, 0), ("tiny", "reverse_id"): (3, 3, 0), ("clique64_hub", "hash"): (65, 65, 1),
    ("clique64_hub", "largest_first"): (65, 65, 1), ("clique64_hub", "smallest_last"): (65, 65, 1), ("clique64_hub", "reverse_id"): (65, 66, 1),
    ("clique64_hub", "own"): (65, 65, 1), ("clique65_hub", "hash"): (66, 66, 2), ("clique65_hub", "largest_first"): (66, 66, 2),
    ("clique65_hub", "smallest_last"): (66, 66, 2), ("clique65_hub", "reverse_id"): (66, 67, 2), ("clique65_hub", "own"): (66, 66, 2)}
# the degeneracy of each case (tests/test_kcore_cpu.py pins those of kcore_ref.CASES against networkx)
DEGENERACY = {"tiny": 2, "star": 1, "hub_leaves_clique": 19, "path": 1, "grid": 2, "doubling_tree": 39, "rmat13": 90, "clique64_hub": 64, "clique65_hub": 65}


@pytest.mark.parametrize("name", ref.CASES)
def test_reference_equals_networkx_greedy_color(name):
    for how in ref.orders_of(name):
        n, rp, ci, key, col, rnd, over = ref.case(name, how)
        assert np.array_equal(col, ref.networkx_color(rp, ci, n, key, 0)), how
        assert (int(col.max()) + 1, int(rnd.max()) + 1, over) == FACTS[name, how], how
        assert ref.is_proper(rp, ci, n, col), how
        assert col.min() == 0 and np.all(col <= ref.higher_neighbours(rp, ci, n, key, 0)), how
        assert ref.class0_is_maximal_independent(rp, ci, n, col), how
        assert rnd.min() == 0 and np.unique(rnd).size == int(rnd.max()) + 1, how                  # every frontier is non-empty
        assert over == int(np.count_nonzero(col >= 64)), how                                       # first fit: colour >= 64 ⇔ 0 … 63 are all held above
    n, rp, ci, key, col, *_ = ref.case(name, "smallest_last")
    assert int(kcore_ref.kcore(rp, ci, n)[0].max()) == DEGENERACY[name]
    assert int(col.max()) + 1 <= DEGENERACY[name] + 1                                              # the textbook bound, for smallest-last only


def test_the_hash_order_may_pass_the_degeneracy_bound():
    assert FACTS["doubling_tree", "hash"][0] == 42 > DEGENERACY["doubling_tree"] + 1


def test_round_is_the_depth_in_the_priority_dag():
    for name, how in (("rmat13", "hash"), ("grid", "smallest_last"), ("clique65_hub", "own")):
        n, rp, ci, key, col, rnd, _ = ref.case(name, how)
        prio = ref.priority(n, key, 0)
        rows = np.repeat(np.arange(n), np.diff(rp))
        up = (ci != rows) & (prio[ci] > prio[rows])
        deepest = np.full(n, -1, np.int64)
        np.maximum.at(deepest, rows[up], rnd[ci[up]])
        assert np.array_equal(rnd, deepest + 1)


def test_each_new_case_has_the_property_it_is_named_for():
    from g4s_amd import capi
    for clique, name in ((64, "clique64_hub"), (65, "clique65_hub")):
        n, rp, ci, key, col, rnd, over = ref.case(name, "own")
        hub = clique
        assert rp[hub + 1] - rp[hub] == clique + 5000 > 4096 and key[hub] == 0 and np.all(np.delete(key, hub) == 1)
        assert sorted(col[:clique].tolist()) == list(range(clique)) and np.all(col[hub + 1:] == 0)   # the clique holds 0 … clique − 1, the leaves 0
        assert col[hub] == clique and rnd[hub] == clique and over == clique - 63                     # the hub: behind a full mask, past the clique
    n, (rp, ci), key = ref.clique_hub(70)
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    assert (int(col[70]), over, int(rnd.max()) + 1) == (70, 7, 71)
    m = 64 + capi.COLOR_WINDOW + 1
    n, (rp, ci), key = ref.clique_window(capi.COLOR_WINDOW)
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    rank = np.empty(m, np.int64)
    rank[ref.order(m)] = np.arange(m)
    assert n == m and np.array_equal(col, rank) and np.array_equal(rnd, rank) and over == m - 64    # K_m: the colour is the rank in priority order
    assert int(col.max()) == 64 + capi.COLOR_WINDOW                                                 # the last vertex: the first colour of the second window


def test_fmix32_against_plain_ints():
    def plain(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    assert plain(0) == 0 and plain(1) == 0x514E28B7                                                # the murmur3 finaliser's known value
    ids = np.array([0, 1, 2, 63, 64, 4095, 4096, 2**31 - 1], np.uint64)
    for seed in (0, 1, 0xDEADBEEF, 2**32 - 1):
        assert ref.fmix32(ids ^ np.uint64(seed)).tolist() == [plain(int(v) ^ seed) for v in ids]
        p = ref.priority(8, None, seed)
        assert [int(x) & 0xFFFFFFFF for x in p] == [plain(v ^ seed) for v in range(8)] and np.unique(p).size == 8
    p = ref.priority(4, np.array([-2**31, 2**31 - 1, 0, -1], np.int32), 5)
    assert np.argsort(p).tolist() == [0, 3, 2, 1]                                                  # any int32 key; the key decides before the hash


def test_struct_constants_and_signature_agree_across_layers():
    from g4s_amd import capi
    text = open(os.path.join(INCLUDE, "g4s.h")).read()
    m = re.search(r"typedef struct g4s_color_info \{(.*?)\} g4s_color_info;", text, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(capi.ColorInfo._fields_)
    assert C.sizeof(capi.ColorInfo) == 48
    assert {"colors", "rounds", "class0", "overflow", "edges_walked", "launches", "resumes", "scan_resumes", "host_waits"} <= {n for n, _ in capi.ColorInfo._fields_}
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text).group(1))
    assert define("G4S_COLOR_LARGEST_FIRST") == capi.COLOR_LARGEST_FIRST == 524288
    assert define("G4S_COLOR_BATCH") == capi.COLOR_BATCH == 16
    assert define("G4S_COLOR_MASK_COLORS") == capi.COLOR_MASK_COLORS == ref.MASK_COLORS == 64
    assert define("G4S_COLOR_WINDOW") == capi.COLOR_WINDOW and capi.COLOR_WINDOW % 32 == 0
    flags = [int(v) for v in re.findall(r"^#define\s+G4S_\w+\s+(\d+)u\b", text, re.M)]
    assert flags.count(524288) == 1 and not any(f & 524288 for f in flags if f != 524288)           # the bit is no other flag's
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"g4s_status\s+g4s_color\s*\((.*?)\);", text, re.S).group(1), flags=re.S)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["int32_t n", "const int32_t *rowptr", "const int32_t *colids", "const int32_t *key", "uint32_t seed", "int32_t *color", "int32_t *round",
                    "unsigned flags", "g4s_color_info *info", "void *stream"]
    vp = C.c_void_p
    assert capi.SIGNATURES["g4s_color"] == (C.c_int, [C.c_int32, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint, C.POINTER(capi.ColorInfo), vp])
    hpp = open(os.path.join(INCLUDE, "g4s", "csr.hpp")).read()
    assert "g4s_color(" in hpp and hpp.count("GreedyColor(") >= 2 and hpp.count("MaximalIndependentSet(") >= 2   # the functions and the header comment's list


def test_symbol_is_exported():
    from g4s_amd import capi
    assert hasattr(capi.load(), "g4s_color")


def test_call_rejects_arguments_before_hip():
    from g4s_amd import capi
    lib = capi.load()
    fn = lib.g4s_color
    fake = C.c_void_p(0x1000)                                         # never dereferenced: every check below comes first
    info = capi.ColorInfo()
    LF = capi.COLOR_LARGEST_FIRST
    for b in [1 << k for k in range(1, 32) if 1 << k != LF] + [1536, 3 << 20, LF | 2]:
        for base in (0, 1):
            assert fn(5, fake, fake, None, 0, fake, fake, base | b, C.byref(info), None) == capi.ERR_INVALID, (base, b)
    assert "flags" in lib.g4s_last_error().decode()
    for f in (0, 1, LF, LF | 1):
        for rnd in (fake, None):
            assert fn(5, None, fake, None, 0, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert fn(5, fake, fake, None, 0, None, rnd, f, None, None) == capi.ERR_INVALID
            assert fn(5, fake, None, None, 0, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert "colids" in lib.g4s_last_error().decode()
            assert fn(-1, fake, fake, None, 0, fake, rnd, f, None, None) == capi.ERR_INVALID
            assert "negative" in lib.g4s_last_error().decode()
            assert fn(0, None, None, None, 0, fake, rnd, f, None, None) == capi.ERR_INVALID       # rowptr is required even for n == 0
    for f in (LF, LF | 1):
        assert fn(5, fake, fake, fake, 0, fake, fake, f, None, None) == capi.ERR_INVALID          # a key together with largest-first
        assert "key" in lib.g4s_last_error().decode()
    # host pointers: outputs that overlap an input or each other (real arrays: the check reads rowptr[n])
    rp, ci, key = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32), np.array([3, 1, 2], np.int32)
    buf = np.zeros(8, np.int32)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + 4 * off)
    for col, rnd in ((P(rp), P(buf)), (P(buf), P(ci)), (P(buf), P(buf, 2)), (P(rp, 3), None), (P(buf), P(buf)), (P(key), None), (P(buf), P(key, 2))):
        assert fn(3, P(rp), P(ci), P(key), 0, col, rnd, capi.HOST_POINTERS, None, None) == capi.ERR_INVALID
        assert "overlap" in lib.g4s_last_error().decode()
    assert rp.tolist() == [0, 1, 2, 2] and ci.tolist() == [1, 0] and key.tolist() == [3, 1, 2] and not buf.any()


def test_cpp_form_compiles(tmp_path):
    src = ("#include \"g4s/csr.hpp\"\n"
           "int main(int argc, char **)\n{\n    g4s::CSR<int32_t, double> a;\n    int32_t c[4], r[4], k[4] = {0, 1, 2, 3};\n    g4s_color_info info = {};\n"
           "    std::vector<char> in_set;\n"
           "    static_assert(sizeof(g4s_color_info) == 48, \"g4s_color_info\");\n"
           "    static_assert(G4S_COLOR_BATCH == 16 && G4S_COLOR_MASK_COLORS == 64 && G4S_COLOR_WINDOW % 32 == 0, \"constants\");\n"
           "    static_assert(G4S_COLOR_LARGEST_FIRST == 524288u, \"G4S_COLOR_LARGEST_FIRST\");\n"
           "    if (argc > 5) { g4s::GreedyColor(a, c); g4s::GreedyColor(a, c, k); g4s::GreedyColor(a, c, k, 7u, r); g4s::GreedyColor(a, c, nullptr, 0, r, true, &info);\n"
           "        g4s::MaximalIndependentSet(a, in_set); g4s::MaximalIndependentSet(a, in_set, k, 3u);\n"
           "        g4s_color(0, nullptr, nullptr, nullptr, 0u, c, r, G4S_DEVICE_POINTERS | G4S_COLOR_LARGEST_FIRST, &info, nullptr); }\n"
           "    return (int)info.class0 * 0 + info.colors * 0 + info.overflow * 0 + info.scan_resumes * 0;\n}\n")
    f = tmp_path / "prog.cpp"
    f.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-c", "-I" + INCLUDE, str(f), "-o", str(tmp_path / "prog.o")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


def test_example_compiles(tmp_path):
    _build_example("color.cpp", str(tmp_path / "color"))


def test_python_value_errors_before_any_gpu_call():
    import torch
    from g4s_amd import host
    wide = types.SimpleNamespace(rows=3, cols=4)                      # no device arrays: the shape is checked first
    square = types.SimpleNamespace(rows=3, cols=3)
    for fn in (host.color, host.CSR.color, host.maximal_independent_set):
        with pytest.raises(ValueError, match="square"):
            fn(wide)
    with pytest.raises(ValueError, match="square"):
        host.color_smallest_last(wide)
    for bad in (-1, 1.0, "3", True, None, 2**32):
        with pytest.raises(ValueError, match="seed"):
            host.color(square, seed=bad)
        with pytest.raises(ValueError, match="seed"):
            host.maximal_independent_set(square, seed=bad)
    for bad in ("yes", 1, 0, None):
        for name in ("largest_first", "return_round", "return_info"):
            with pytest.raises(ValueError, match=name):
                host.color(square, **{name: bad})
    with pytest.raises(ValueError, match="largest_first"):
        host.color(square, key=np.zeros(3, np.int32), largest_first=True)
    rp, ci = np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32)
    with pytest.raises(ValueError, match="one value per vertex"):
        host.color((rp, ci), key=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="kind"):
        host.color((rp, ci), key=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="pair"):
        host.color((np.zeros(1, np.int32),))
    with pytest.raises(ValueError, match="rowptr"):
        host.color((np.zeros(0, np.int32), np.zeros(0, np.int32)))
    for bad in (np.zeros(3, np.int32), torch.zeros(3, dtype=torch.int64), torch.zeros((3, 1), dtype=torch.int32), None):
        with pytest.raises(ValueError, match="int32"):
            host.color_classes(bad)
