"""The cases of tests/graph_cases.py cover every instantiation the restated selection rules can produce, have the properties their names claim,
sit on the claimed side of every threshold (all integer comparisons: one off is exact), and the oracle's result on each equals a numpy.longdouble
restatement of the operation (1e-14·Σ|terms| on real data, equality on integer data) — so that tests/test_graph_kernels_gpu.py compares the device
with a checked reference on checked inputs. No GPU."""
import numpy as np
import pytest

from tests import graph_cases as gc

DENSE = [c.name for c in gc.dense_cases()]
SMALL_DENSE = [c.name for c in gc.dense_cases() if not c.claims.get("big")]
ELEM = [c.name for c in gc.elem_cases()]
RUN_ELEM = [c.name for c in gc.elem_cases() if c.kernel != "refused"]
QUAD = [c.name for c in gc.quad_cases()]


# ------------------------------------------------------------------------------------------------ the restated rules at hand-worked points
def test_restated_rules_at_hand_worked_points():
    """Values worked out by hand from graph.hip, so that a slip in the restatement does not pass for a property of the library."""
    assert gc.forward_dispatch(4096, 100, 100) == {"kernel": "resident2", "KT": 7, "GT": 13, "WT": 0, "grid": 32}
    assert gc.forward_dispatch(70000, 100, 100, wt=True) == {"kernel": "resident2", "KT": 7, "GT": 13, "WT": 1, "grid": 256}
    assert gc.forward_dispatch(10007, 37, 50) == {"kernel": "resident", "KT": 4, "NS": 10, "WT": 0, "grid": 79}
    assert gc.forward_dispatch(5000, 128, 128) == {"kernel": "panel", "WT": 0, "grid": 79}
    assert gc.forward_dispatch(29, 13, 7) == {"kernel": "panel", "WT": 0, "grid": 1}
    # the 96 KiB bound of the older resident kernel: 8 bytes · 4·NS · 16·KT
    assert 8 * 4 * 24 * 128 == gc.RESIDENT_LDS and 8 * 4 * 25 * 128 > gc.RESIDENT_LDS          # N = 96 | 97 at K = 128
    assert 8 * 4 * 27 * 112 <= gc.RESIDENT_LDS < 8 * 4 * 28 * 112                                # N = 108 | 109 at K = 112
    assert 8 * 4 * 32 * 96 == gc.RESIDENT_LDS and 8 * 4 * 32 * 112 > gc.RESIDENT_LDS            # K = 96 | 97 at N = 128
    # every resident2 instantiation fits its own bound: the LDS test never decides
    assert max(8 * 8 * gt * 16 * kt for kt, gt in gc.R2_PAIRS) == 8 * 8 * 13 * 16 * 8 <= gc.RESIDENT2_LDS
    assert gc.dw_geometry(8192, 20, 20) == {"KT": 2, "rows_per_wg": 16, "ranges": 512, "by": 1, "bz": 1}
    assert gc.dw_geometry(8193, 20, 20) == {"KT": 2, "rows_per_wg": 32, "ranges": 257, "by": 1, "bz": 1}
    assert 8193 - 256 * 32 == 1                                                                  # the last range holds one row
    assert gc.dw_geometry(40, 130, 257) == {"KT": 8, "rows_per_wg": 16, "ranges": 3, "by": 2, "bz": 3}
    assert gc.strip_iterations(4096) == (1, 256) and gc.strip_iterations(32768) == (1, 2048) and gc.strip_iterations(32769) == (2, 1)
    assert [gc.dw_row_tiles(N, 0, 0) for N in (1, 16, 17, 64, 65, 128)] == [1, 1, 1, 1, 2, 2]
    assert [gc.dw_row_tiles(65, 0, w) for w in range(4)] == [2, 1, 1, 1] and [gc.dw_row_tiles(17, 0, w) for w in range(4)] == [1, 1, 0, 0]
    assert gc.dw_row_tiles(129, 1, 0) == 1 and gc.dw_row_tiles(129, 1, 1) == 0


# ------------------------------------------------------------------------------------------------ coverage
def test_the_cases_cover_every_instantiation():
    fwd = [c.dispatch() for c in gc.dense_cases() if c.dispatch() is not None]
    r2 = {(d["KT"], d["GT"], d["WT"]) for d in fwd if d["kernel"] == "resident2"}
    assert r2 == {(kt, gt, wt) for kt, gt in gc.R2_PAIRS for wt in (0, 1)} and len(r2) == 28
    assert {(d["KT"], d["WT"]) for d in fwd if d["kernel"] == "resident"} == {(kt, wt) for kt in range(1, 9) for wt in (0, 1)}
    assert {d["WT"] for d in fwd if d["kernel"] == "panel"} == {0, 1}
    dws = [c.dw() for c in gc.dense_cases() if c.dw() is not None]
    assert {d["KT"] for d in dws} == set(range(1, 9))
    assert any(d["by"] > 1 and d["bz"] > 1 for d in dws), "a block of dw with blockIdx.y and blockIdx.z both above 0"
    # the exhaustive rule over the whole persistent range produces nothing the cases do not hold
    seen_r2, seen_res = set(), set()
    for N in range(0, 131):
        for K in range(1, 131):
            d = gc.forward_dispatch(4096, N, K)
            if d["kernel"] == "resident2":
                seen_r2.add((d["KT"], d["GT"]))
            elif d["kernel"] == "resident":
                seen_res.add(d["KT"])
    assert seen_r2 == set(gc.R2_PAIRS) and seen_res == set(range(1, 9))


def test_resident2_cases_sit_at_the_ends_of_their_ranges():
    n_ends, k_ends, rows = {}, {}, set()
    for kt, gt in gc.R2_PAIRS:
        for suffix in ("fwd", "dxx"):
            c = gc.dense_case(f"r2_kt{kt}_gt{gt}_{suffix}")
            N, K = (c.N, c.K) if suffix == "fwd" else (c.K, c.N)
            assert N in gc.R2_N[gt] and K in gc.R2_K[kt] and N % 2 == 0
            lo_n, hi_n = gc.R2_N[gt]
            assert 8 * gt - lo_n >= 2 and hi_n == 8 * gt               # low: at least one pair of the last group lies past N; high: none
            lo_k, hi_k = gc.R2_K[kt]
            assert lo_k == 16 * (kt - 1) + 1 and hi_k == 16 * kt       # low: one real column in the last tile
            n_ends.setdefault(gt, set()).add(gc.R2_N[gt].index(N))
            k_ends.setdefault(kt, set()).add(gc.R2_K[kt].index(K))
            rows.add(c.M)
    assert all(v == {0, 1} for v in n_ends.values()) and all(v == {0, 1} for v in k_ends.values())
    assert rows == {4096, 4111} and 4111 % 16 != 0                    # 4111: the row clamp and the dump slot


# ------------------------------------------------------------------------------------------------ dense claims
@pytest.mark.parametrize("name", DENSE)
def test_dense_case_has_its_claimed_properties(name):
    c = gc.dense_case(name)
    d = c.dispatch()
    if c.kernel is None:
        assert d is None and c.claims.get("untouched") and (c.M == 0 or c.K == 0)
        return
    assert d["kernel"] == c.kernel, d
    for key, val in c.targs.items():
        assert d[key] == val, d
    assert d["WT"] == (c.mode == "grad")
    assert set(c.targs) == {"resident2": {"KT", "GT"}, "resident": {"KT"}, "panel": set()}[c.kernel]
    M, N, K = (c.M, c.N, c.K) if c.mode == "forward" else (c.M, c.K, c.N)           # the product as the launcher sees it
    cl = c.claims
    if "lds" in cl:
        assert 8 * 4 * d["NS"] * 16 * d["KT"] == cl["lds"]
    if cl.get("zero_result"):
        assert N == 0
    if "iterations" in cl:
        most, waves = gc.strip_iterations(M)
        assert most == cl["iterations"] == gc.STRIP_M[M] and 0 < waves < 8 * gc.PERSIST_GRID and d["grid"] == gc.PERSIST_GRID
    if "last_pass_cols" in cl:
        assert K > gc.PANEL_COLS and (K - 1) % gc.PANEL_COLS + 1 == cl["last_pass_cols"] and cl["last_pass_cols"] in (1, 16, 17)
    dw = c.dw()
    for key in ("KT", "rows_per_wg", "ranges", "by", "bz"):
        if "dw_" + key in cl:
            assert dw[key] == cl["dw_" + key], dw
    if "dw_last_rows" in cl:
        assert (c.N - 1) % gc.DW_BLOCK + 1 == cl["dw_last_rows"] and cl["dw_last_rows"] in (1, 16, 17, 64, 65, 128)
    if c.claims.get("big"):
        assert c.M * max(c.N, c.K) * 8 <= 22e6                       # the largest operand stays about 20 MB


def test_dense_cases_named_in_the_plan_exist():
    have = {(c.mode, c.M, c.N, c.K, c.misaligned): c for c in gc.dense_cases()}
    for M, N, K, kernel in ((4095, 100, 100, "panel"), (4096, 96, 128, "resident"), (4096, 97, 128, "panel"), (4096, 108, 112, "resident"),
                            (4096, 109, 112, "panel"), (4096, 128, 96, "resident"), (4096, 128, 97, "panel"), (4096, 128, 128, "panel"),
                            (4096, 122, 113, "panel"), (4096, 129, 20, "panel"), (4096, 20, 129, "panel"), (4096, 24, 17, "resident"),
                            (4111, 33, 65, "resident")):
        assert have[("forward", M, N, K, False)].kernel == kernel
        assert have[("grad", M, K, N, False)].kernel == kernel
    assert have[("forward", 4096, 128, 96, False)].targs == {"KT": 6}
    assert have[("forward", 4111, 26, 17, True)].kernel == "resident" and have[("forward", 4111, 26, 17, False)].kernel == "resident2"
    for M in gc.STRIP_M:
        for N, kernel in ((26, "resident2"), (27, "resident")):
            assert have[("forward", M, N, 17, False)].kernel == kernel and have[("grad", M, 17, N, False)].kernel == kernel
    grads = [c for c in gc.dense_cases() if c.mode == "grad"]
    for kt in range(1, 9):
        assert {c.K for c in grads if c.M == 100 and c.N == 20} >= {16 * kt - 15, 16 * kt}
    assert {c.K for c in grads if c.M == 100 and c.N == 20} >= {129, 257}
    assert {c.N for c in grads if c.M == 50 and c.K == 20} == {1, 16, 17, 64, 65, 128, 129, 144, 145, 192, 193, 256}
    assert any(c.N == 130 and c.K == 130 for c in grads)
    assert {c.M for c in grads if c.N == 20 and c.K == 20} >= {1, 15, 16, 17, 33, 8191, 8192, 8193, 16385, 40000}
    fwd = [c for c in gc.dense_cases() if c.mode == "forward" and c.kernel == "panel" and c.M < 4096]
    assert {c.K for c in fwd} >= {129, 144, 145, 257} and {c.N for c in fwd} >= {0, 1, 3, 4, 5, 64, 65, 130} and {c.M for c in fwd} >= {1, 63, 64, 65}


@pytest.mark.parametrize("a,b", gc.DENSE_THRESHOLD_PAIRS)
def test_threshold_pairs_differ_by_one(a, b):
    for suffix in ("_fwd", "_dxx"):
        ca, cb = gc.dense_case(a + suffix), gc.dense_case(b + suffix)
        diff = [abs(x - y) for x, y in zip((ca.M, ca.N, ca.K), (cb.M, cb.N, cb.K))]
        assert sorted(diff) == ([0, 0, 1] if ca.misaligned == cb.misaligned else [0, 0, 0])
        assert ca.dispatch()["kernel"] != cb.dispatch()["kernel"]
        assert (ca.dispatch()["kernel"], cb.dispatch()["kernel"]) == (ca.kernel, cb.kernel)


def test_dw_range_split_steps():
    """M = 15 / 16 / 17: one range, one full range, a second range of one row; 8192 / 8193: rows_per_wg goes from 16 to 32."""
    g = lambda M: gc.dw_geometry(M, 20, 20)
    assert [g(M)["ranges"] for M in (15, 16, 17)] == [1, 1, 2] and 17 - 16 == 1
    assert (g(8192)["rows_per_wg"], g(8193)["rows_per_wg"]) == (16, 32)
    assert 8193 - (g(8193)["ranges"] - 1) * 32 == 1


# ------------------------------------------------------------------------------------------------ element meshes
@pytest.mark.parametrize("name", ELEM)
def test_elem_case_has_its_claimed_properties(name):
    c, m = gc.elem_case(name), gc.mesh(name)
    assert m.ien.dtype == np.int32 and m.id.dtype == np.int32 and m.ien.shape[1] == m.npe and m.id.shape == (m.nno, m.dof)
    assert m.ien.min() >= 0 and m.ien.max() < m.nno
    assert m.id.min() >= 0 and m.id.max() < m.neq and len(np.unique(m.id)) == m.id.size, "every equation has at most one owner"
    assert all(len(set(row)) == m.npe for row in m.ien.tolist()), "the nodes of an element are distinct"
    cl = c.claims
    assert m.npe * m.dof == cl["n"]
    d = gc.elem_dispatch(m.ien, m.nno, m.npe, m.dof)
    if c.kernel == "refused":
        assert m.dof > gc.ELEM_MAX_DOF
        return
    assert m.dof <= gc.ELEM_MAX_DOF and d["kernel"] == c.kernel
    mt = gc.max_terms(m.ien, m.nno)
    if "max_terms" in cl:
        assert mt == cl["max_terms"]
    if "rounds" in cl:
        assert -(-mt // gc.ELEM_TERMS_PER_ROUND) == cl["rounds"]
    if c.kernel == "fixed8":
        assert (m.npe, m.dof) == (8, 3) and mt <= 8
    else:
        assert (d["npe"], d["dof"], d["max_terms"]) == (m.npe, m.dof, mt)
    unowned = m.neq - m.nno * m.dof
    assert unowned == cl.get("unowned", 0)
    if "unreferenced" in cl:
        assert m.nno - len(np.unique(m.ien)) >= cl["unreferenced"] > 0
    if "nno" in cl:
        assert m.nno == cl["nno"] and m.nno % gc.ELEM_NODES_PER_WG != 0


def test_elem_cases_named_in_the_plan_exist():
    by = {c.name: c for c in gc.elem_cases()}
    assert [by[f"tet_fan_{T}"].claims["rounds"] for T in (1, 8, 9, 16, 17, 25)] == [1, 1, 2, 2, 3, 4]
    assert by["hex_fan_8"].kernel == "fixed8" and by["hex_fan_9"].kernel == "generic"
    shapes = {(gc.mesh(n).npe, gc.mesh(n).dof) for n in by}
    assert shapes >= {(8, 1), (8, 2), (8, 4), (3, 3), (1, 1), (27, 3), (4, 3), (8, 3), (2, 5)}
    assert {gc.mesh(n).dof for n in by if by[n].kernel == "generic"} == {1, 2, 3, 4}
    assert {gc.mesh(n).npe * gc.mesh(n).dof % 8 for n in by if by[n].kernel == "generic"} >= {0, 1, 4}     # the c += 8 column loop's tails
    assert {gc.mesh(n).nno for n in by} >= {1, 2, 3, 5}
    assert by["scattered_hex"].kernel == "fixed8" and by["scattered_tet"].kernel == "generic"


def test_quad_cases_named_in_the_plan_exist():
    cs = gc.quad_cases()
    assert {(c.m, c.numbers, c.with_b) for c in cs} == {(m, n, b) for m in (1, 2, 255, 256, 257, 513) for n, b in ((1, False), (1, True), (2, False), (3, False))}
    assert {-(-c.m // gc.QUAD_THREADS) for c in cs} == {1, 2, 3}     # steps of the i += 256 stride
    for c in cs:
        a, x, b = gc.quad_operands(c, "real")
        assert a.min() < 0 < a.max() or c.m == 1
        assert len(a) == c.m * c.m * c.numbers and (b is not None) == c.with_b
    a, x, _ = gc.quad_operands(cs[-1], "int")
    assert a.min() == -3 and a.max() == 3 and np.array_equal(a, np.round(a))


def test_integer_sums_stay_exact():
    """The largest possible |sum| of the integer cases is far below 2^53."""
    assert max(c.M * 9 for c in gc.dense_cases()) < 2 ** 24 and max(max(c.N, c.K) * 9 for c in gc.dense_cases()) < 2 ** 24
    assert 2 * 513 * 513 * 27 < 2 ** 24 and 25 * 81 * 9 < 2 ** 24


# ------------------------------------------------------------------------------------------------ the oracle against longdouble
def _agree(got, want_ld, scale, kind, what):
    if kind == "int":
        assert np.array_equal(got, want_ld.astype(np.float64)), what
    else:
        err = np.abs(got.astype(gc.LD) - want_ld)
        assert np.all(err <= 1e-14 * scale + 1e-300), (what, float(np.max(err / (scale + 1e-300))))


@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("name", SMALL_DENSE)
def test_oracle_dense_agrees_with_longdouble(oracle, name, kind):
    c = gc.dense_case(name)
    ops = gc.dense_operands(c, kind)
    if c.mode == "forward":
        xx, w = ops
        _agree(gc.oracle_dense(oracle, xx, w), gc.ld_dense(xx, w), gc.dense_scale(xx, w), kind, name)
    else:
        xx, w, grad = ops
        dxx, dw = oracle.dense_rows_times_matrix_grad(xx, w, grad)
        want_dxx, want_dw = gc.ld_dense_grad(xx, w, grad)
        s_dxx, s_dw = gc.dense_grad_scales(xx, w, grad)
        _agree(dxx, want_dxx, s_dxx, kind, name + " dxx")
        _agree(dw, want_dw, s_dw, kind, name + " dw")


@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("name", RUN_ELEM)
def test_oracle_element_matvec_agrees_with_longdouble(oracle, name, kind):
    m = gc.mesh(name)
    K, u = gc.elem_operands(name, kind)
    for base in (0, 1):
        got = oracle.element_matvec(m.ien, m.id, K, u, m.neq, npe=m.npe, dof=m.dof, base=base)
        _agree(got, gc.ld_element_matvec(m, K, u), gc.elem_scale(m, K, u), kind, name)
    owned = np.zeros(m.neq, bool)
    owned[m.id.ravel()] = True
    assert np.all(got[~owned] == 0.0)


@pytest.mark.parametrize("name", QUAD)
def test_oracle_quadratic_form_agrees_with_longdouble_on_integers(oracle, name):
    """Integer data only: the oracle's sequential sum of the 131 000 terms at m = 513 cannot promise 1e-12 on real data, so there the longdouble
    restatement is the reference of the GPU test and the oracle is not used."""
    c = {q.name: q for q in gc.quad_cases()}[name]
    a, x, b = gc.quad_operands(c, "int")
    got = oracle.sym_quadratic_form(c.m, c.numbers, a, x, b if b is not None else np.zeros(c.m))
    assert np.array_equal(got, gc.ld_sym_quadratic_form(c.m, c.numbers, a, x, b).astype(np.float64))


def test_longdouble_quadratic_form_is_the_definition():
    """The vectorised restatement against the double loop of the definition, and its magnitudes against |terms| summed one by one."""
    c = gc.QuadCase("loop_check", 7, 3, False)
    a, x, _ = gc.quad_operands(c, "real")
    want, mag = np.zeros(2, gc.LD), np.zeros(2, gc.LD)
    al, xl = a.astype(gc.LD), x.astype(gc.LD)
    for s in (0, 1):
        for i in range(7):
            for j in range(i):
                t = xl[i] * xl[j] * (al[3 * (i + 7 * j) + s] + al[3 * (j + 7 * i) + s])
                want[s] += t
                mag[s] += abs(xl[i] * xl[j]) * (abs(al[3 * (i + 7 * j) + s]) + abs(al[3 * (j + 7 * i) + s]))
            want[s] += xl[i] * xl[i] * al[3 * (i + 7 * i) + s]
            mag[s] += xl[i] * xl[i] * abs(al[3 * (i + 7 * i) + s])
    assert np.allclose(gc.ld_sym_quadratic_form(7, 3, a, x).astype(float), want.astype(float), rtol=1e-15, atol=1e-17)
    assert np.allclose(gc.ld_sym_quadratic_form(7, 3, a, x, magnitudes=True).astype(float), mag.astype(float), rtol=1e-15, atol=0)
