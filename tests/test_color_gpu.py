"""g4s_color on the device. Every comparison is exact: colours, rounds and the overflow count are functions of the graph and the priorities alone, so they
are compared with == against tests/color_ref.py (pinned to networkx.greedy_color in test_color_cpu.py). Each case runs under four orders, with device and
with host pointers, with pre-filled outputs, with `round` given and NULL, and every call runs twice with equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import color_ref as ref
from tests import kcore_ref

pytestmark = pytest.mark.gpu

FILL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).cuda()            # a copy: the shared cases are read-only


def _call(rp, ci, n, key=None, seed=0, largest=False, device=True, with_round=True, stream=None, check=True):
    """The C entry point itself, outputs pre-filled: (color, round or None, info dict, status)."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.ColorInfo()
    flags = capi.COLOR_LARGEST_FIRST if largest else 0
    if device:
        rp_t, ci_t = (rp if isinstance(rp, torch.Tensor) else _dev(rp)), (ci if isinstance(ci, torch.Tensor) else _dev(ci))
        key_t = None if key is None else key if isinstance(key, torch.Tensor) else _dev(key)
        col = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        rnd = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        st = lib.g4s_color(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), host._ptr_nn(key_t) if key_t is not None and n else None, seed, host._ptr_nn(col),
                           host._ptr_nn(rnd) if with_round else None, flags | capi.DEVICE_POINTERS, C.byref(info), s)
        if stream is not None:
            stream.synchronize()
        col, rnd = col.cpu().numpy(), rnd.cpu().numpy()
    else:
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        key_h = None if key is None else np.ascontiguousarray(key, np.int32)
        col, rnd = np.full(max(n, 1), FILL, np.int32), np.full(max(n, 1), FILL, np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.g4s_color(n, P(rp_h), P(ci_h if ci_h.size else col), P(key_h) if key_h is not None and n else None, seed, P(col), P(rnd) if with_round else None,
                           flags | capi.HOST_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        capi.check(st)
    if not with_round:
        assert np.all(rnd == FILL)                                    # a NULL round: nothing is written anywhere near
    return col[:n], (rnd[:n] if with_round else None), {k: getattr(info, k) for k, _ in capi.ColorInfo._fields_}, st


def _check_info(info, rp, ci, n, col, rnd, over):
    assert (info["colors"], info["rounds"], info["class0"], info["overflow"]) == (int(col.max()) + 1, int(rnd.max()) + 1, int(np.count_nonzero(col == 0)), over), info
    assert info["edges_walked"] == int(kcore_ref.degrees(rp, ci, n).sum()), info                   # every row is walked once
    assert info["host_waits"] <= info["launches"] // 16 + 2 + info["resumes"] + info["scan_resumes"], info
    assert info["scan_resumes"] == int(over > 0), info                                             # the scan joins once, and only when a mask filled up


def _exact(rp, ci, n, key, col, rnd, over, seed=0, largest=False, streams=(None,)):
    """both pointer kinds, round given and NULL, twice each: the reference's bits and the reference's counts"""
    infos = []
    dev = (_dev(rp), _dev(ci), None if key is None or largest else _dev(key))
    host_key = None if largest else key
    for device in (True, False):
        for with_round in (True, False):
            for stream in streams:
                for _ in range(2):
                    a = dev if device else (rp, ci, host_key)
                    c, r, info, _ = _call(a[0], a[1], n, key=a[2], seed=seed, largest=largest, device=device, with_round=with_round, stream=stream)
                    assert np.array_equal(c, col), (device, with_round)
                    assert r is None or np.array_equal(r, rnd), (device, with_round)
                    _check_info(info, rp, ci, n, col, rnd, over)
                    infos.append(info)
    return infos


@pytest.mark.parametrize("name", ref.CASES)
def test_case_equals_reference(name):
    for how in ref.orders_of(name):
        n, rp, ci, key, col, rnd, over = ref.case(name, how)
        infos = _exact(rp, ci, n, key, col, rnd, over, largest=how == "largest_first")             # largest-first: the call works the key out itself
        print(f"{name} {how}: {infos[0]}")
        if name == "grid":
            assert all(i["scan_resumes"] == 0 and i["overflow"] == 0 for i in infos)               # below 65 colours the scan never enters
        if name in ref.HUB_CASES and how == "own":
            assert all(i["scan_resumes"] == 1 and i["overflow"] == over for i in infos)


def test_another_seed_is_another_order():
    n, rp, ci, _, col0, _, _ = ref.case("rmat13", "hash")
    n, rp, ci, key, col, rnd, over = ref.case("rmat13", "hash", 0x9E3779B9)
    assert not np.array_equal(col, col0)
    _exact(rp, ci, n, key, col, rnd, over, seed=0x9E3779B9)


def test_a_long_chain_doubles_the_batch():
    """path with key = n − 1 − id: 4001 dependent steps. The batches run 16, 32 and then 64 launches, so the call waits about once per 64 steps."""
    n, rp, ci, key, col, rnd, over = ref.case("path", "reverse_id")
    assert int(rnd.max()) + 1 == 4001 == n
    for device in (True, False):
        c, r, info, _ = _call(rp, ci, n, key=key, device=device)
        assert np.array_equal(c, col) and np.array_equal(r, rnd)
        _check_info(info, rp, ci, n, col, rnd, over)
        assert info["launches"] >= 4001 and info["host_waits"] <= 4001 // 64 + 8, info            # 1 behind the seed, 2 for the first 48 steps, one per 64 after, 1 for the copies


@pytest.mark.parametrize("hub_first", (True, False))
def test_star_with_the_hub_first_and_last(hub_first):
    """The hub first: a row above the hub cut in the walk, 5000 vertices released at once. The hub last: 5000 decrements and one mask bit on one word."""
    n, (rp, ci) = kcore_ref.star()
    key = np.full(n, 0 if hub_first else 1, np.int32)
    key[0] = 1 if hub_first else 0
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    assert rp[1] - rp[0] == 5000 > 4096 and col[0] == (0 if hub_first else 1) and rnd[0] == (0 if hub_first else 1) and np.all(col[1:] == (1 if hub_first else 0))
    _exact(rp, ci, n, key, col, rnd, over)


def test_the_frontier_outgrows_the_launch_grid():
    """A doubling tree coloured root first (key = −depth): the frontier at depth d has 3 · 2^d entries, which at depth 16 passes the 8 · 8 · 2048 = 131072
    that the smallest grid's batch takes; the batch stops and resumes on a larger grid."""
    n, (rp, ci) = kcore_ref.doubling_tree(17)
    tree = (1 << 18) - 1
    key = np.full(n, -18, np.int32)                                   # the clique behind the leaves
    key[:tree] = -np.floor(np.log2(np.arange(1, tree + 1))).astype(np.int32)
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    assert np.array_equal(rnd[:tree], -key[:tree]) and int(np.diff(rp)[rnd == 16].sum()) == 3 << 16 > 8 * 8 * 2048
    for device in (True, False):
        for _ in range(2):
            c, r, info, _ = _call(rp, ci, n, key=key, device=device)
            assert np.array_equal(c, col) and np.array_equal(r, rnd)
            _check_info(info, rp, ci, n, col, rnd, over)
            assert info["resumes"] >= 1, info
    print(f"doubling tree of depth 17: {info}")


def test_the_row_scan_needs_a_second_window():
    from g4s_amd import capi
    n, (rp, ci), key = ref.clique_window(capi.COLOR_WINDOW)
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    assert int(col.max()) == 64 + capi.COLOR_WINDOW and over == capi.COLOR_WINDOW + 1
    infos = _exact(rp, ci, n, key, col, rnd, over)
    assert all(i["scan_resumes"] == 1 and i["overflow"] == over for i in infos)


@pytest.fixture(scope="module")
def hubby():
    """The smallest symmetrised R-MAT of the library's own generator (edge factor 16) whose longest row passes 4096 entries, as in tests/test_kcore_gpu.py:
    long rows and overflow in the middle of a real run. (scale, CSR on the device, host arrays, the peel round for the smallest-last key)"""
    from g4s_amd import host
    for scale in range(14, 21):
        n = 1 << scale
        A = host.csr_symmetrise(host.rmat_csr(n, scale, 16 * n, 20240613))
        rp = A.rowptr.cpu().numpy()
        if int(np.diff(rp).max()) > 4096:
            ci = A.colids.cpu().numpy()
            return scale, A, rp, ci, kcore_ref.kcore(rp, ci, n)[1].astype(np.int32)
    raise AssertionError("no R-MAT up to scale 20 has a row above 4096 entries")


@pytest.mark.parametrize("how", ("hash", "smallest_last"))
def test_larger_rmat_has_hubs_and_overflow_in_the_middle_of_the_run(hubby, how):
    scale, A, rp, ci, peel = hubby
    n = A.rows
    key = peel if how == "smallest_last" else None
    col, rnd, over = ref.color(rp, ci, n, key, 0)
    longest = int(np.argmax(np.diff(rp)))
    assert rp[longest + 1] - rp[longest] > 4096
    if how == "hash":
        assert over > 0 and rnd[col >= 64].min() >= 64 and np.any(np.diff(rp)[col >= 64] > 4096)   # masks fill up while the run is under way, a hub's among them
    key_t = None if key is None else _dev(key)
    for device in (True, False):
        for with_round in (True, False):
            for _ in range(2):
                c, r, info, _ = _call(A.rowptr if device else rp, A.colids if device else ci, n, key=key_t if device else key, device=device, with_round=with_round)
                assert np.array_equal(c, col) and (r is None or np.array_equal(r, rnd))
                _check_info(info, rp, ci, n, col, rnd, over)
    print(f"rmat{scale} {how}: longest row {rp[longest + 1] - rp[longest]}, round of the longest row {rnd[longest]}, {info}")
    got, got_r, got_info = A.color(key=key_t, return_round=True, return_info=True)
    assert np.array_equal(got.cpu().numpy(), col) and np.array_equal(got_r.cpu().numpy(), rnd) and got_info["overflow"] == over


def test_the_smallest_grid_does_not_change_the_outputs(monkeypatch):
    n, (rp, ci) = kcore_ref.doubling_tree(15)
    col, rnd, over = ref.color(rp, ci, n, None, 0)
    cases = [(n, rp, ci, None, col, rnd, over)] + [ref.case("rmat13", "hash"), ref.case("clique65_hub", "own")]
    for grid in ("1", "64"):
        monkeypatch.setenv("G4S_COLOR_MIN_GRID", grid)
        for n, rp, ci, key, col, rnd, over in cases:
            c, r, info, _ = _call(rp, ci, n, key=key)
            assert np.array_equal(c, col) and np.array_equal(r, rnd), grid
            _check_info(info, rp, ci, n, col, rnd, over)


def _refusal_cases():
    n, rp, ci, _ = ref.graph("grid")
    descending, outside, shifted = ci.copy(), ci.copy(), rp.copy()
    r = 70                                                            # an interior row: four entries
    descending[rp[r]], descending[rp[r] + 1] = ci[rp[r] + 1], ci[rp[r]]
    outside[rp[r] + 3] = n
    shifted[0] = 1
    return {"a descending row": (rp, descending, "ascending"), "an id = n": (rp, outside, "outside"), "rowptr[0] != 0": (shifted, ci, "rowptr")}


def test_refusals_leave_the_thread_and_stream_usable():
    """Each refusal is followed by an exact call on the same thread and stream (the recovery rule of tests/test_readback_recovery_gpu.py)."""
    from g4s_amd import capi
    lib = capi.load()
    n, rp, ci, key, col, rnd, over = ref.case("grid", "hash")
    stream = torch.cuda.Stream()
    for what, (brp, bci, word) in _refusal_cases().items():
        for device in (True, False):
            _, _, _, st = _call(brp, bci, n, device=device, stream=stream, check=False)
            assert st == capi.ERR_INVALID and word in lib.g4s_last_error().decode(), (what, device, lib.g4s_last_error().decode())
            c, r, info, _ = _call(rp, ci, n, device=device, stream=stream)
            assert np.array_equal(c, col) and np.array_equal(r, rnd), (what, device)
            _check_info(info, rp, ci, n, col, rnd, over)


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, key, col, rnd, over = ref.case("grid", "hash")
    rp_t, ci_t = _dev(rp), _dev(ci)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    out_r = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    info = capi.ColorInfo()
    info.rounds = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_color(n, host._ptr(rp_t), host._ptr(ci_t), None, 0, host._ptr(out), host._ptr(out_r), capi.DEVICE_POINTERS, C.byref(info),
                           C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.rounds == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(out == FILL) and torch.all(out_r == FILL)       # nothing was enqueued
    c, r, _, _ = _call(rp_t, ci_t, n, stream=stream)                 # and the library still works, on that stream too
    assert np.array_equal(c, col) and np.array_equal(r, rnd)


def test_python_forms_and_empty_inputs():
    from g4s_amd import host
    n, rp, ci, key, col, rnd, over = ref.case("tiny", "reverse_id")
    A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
    assert A.color(key=_dev(key)).cpu().numpy().tolist() == col.tolist()
    c, r = host.color((rp, ci), key=key, return_round=True)          # numpy arrays: host pointers
    assert c.is_cuda and c.cpu().numpy().tolist() == col.tolist() and r.cpu().numpy().tolist() == rnd.tolist()
    c, info = host.color((_dev(rp), _dev(ci)), largest_first=True, return_info=True)
    want = ref.case("tiny", "largest_first")
    assert c.cpu().numpy().tolist() == want[4].tolist() and (info["colors"], info["rounds"], info["overflow"]) == (3, 3, 0) and "reserved" not in info
    for device in (True, False):
        for largest in (False, True):
            c, r, info, _ = _call(np.zeros(1, np.int32), np.zeros(0, np.int32), 0, largest=largest, device=device)   # n == 0: nothing is written
            assert c.size == 0 and info["launches"] == 0 and info["rounds"] == 0 and info["colors"] == 0
            m = 1000
            c, r, info, _ = _call(np.zeros(m + 1, np.int32), np.zeros(0, np.int32), m, largest=largest, device=device)   # nnz == 0: every colour 0, every round 0
            assert not c.any() and not r.any() and (info["colors"], info["rounds"], info["class0"], info["overflow"], info["edges_walked"]) == (1, 1, m, 0, 0)
            c, r, info, _ = _call(np.array([0, 1], np.int32), np.array([0], np.int32), 1, largest=largest, device=device)   # one vertex with a self-loop
            assert c.tolist() == [0] and r.tolist() == [0] and info["edges_walked"] == 0


def test_classes_independent_set_and_smallest_last():
    from g4s_amd import host
    for name in ("rmat13", "hub_leaves_clique", "grid"):
        n, rp, ci, _, col, rnd, over = ref.case(name, "hash")
        A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
        c = host.color(A)
        assert np.array_equal(c.cpu().numpy(), col)
        mis = host.maximal_independent_set(A)
        assert mis.dtype == torch.bool and np.array_equal(mis.cpu().numpy(), col == 0)
        perm, offsets = host.color_classes(c)
        want_perm, want_offsets = ref.classes(col)
        assert perm.dtype == torch.int32 and np.array_equal(perm.cpu().numpy(), want_perm) and np.array_equal(offsets.cpu().numpy(), want_offsets)
        B = host.csr_permute(A, perm)
        brp, bci = B.rowptr.cpu().numpy(), B.colids.cpu().numpy()
        rows = np.repeat(np.arange(n), np.diff(brp))
        block = np.searchsorted(want_offsets, np.arange(n), side="right") - 1
        off = rows != bci
        assert not np.any(block[rows[off]] == block[bci[off]])        # no stored off-diagonal entry inside a diagonal block: a class is independent
        sl, info = host.color_smallest_last(A, return_info=True)
        _, kinfo = host.kcore(A, return_info=True)
        want = ref.case(name, "smallest_last")
        assert np.array_equal(sl.cpu().numpy(), want[4]) and info["colors"] <= kinfo["degeneracy"] + 1
