"""g4s_kcore on the device. Every comparison is exact: core numbers and peel rounds are a function of the graph alone, so they are compared with ==
against tests/kcore_ref.py (pinned to networkx.core_number in test_kcore_cpu.py). Each case runs with device and with host pointers, with pre-filled
outputs, with `round` given and NULL, and every call runs twice with equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kcore_ref as ref

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
FILL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).cuda()            # a copy: the shared cases are read-only


def _call(rp, ci, n, max_k=INT32_MAX, device=True, with_round=True, stream=None, check=True):
    """The C entry point itself, outputs pre-filled: (core, round or None, info dict, status)."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.KCoreInfo()
    if device:
        rp_t, ci_t = (rp if isinstance(rp, torch.Tensor) else _dev(rp)), (ci if isinstance(ci, torch.Tensor) else _dev(ci))
        core = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        rnd = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        st = lib.g4s_kcore(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), max_k, host._ptr_nn(core), host._ptr_nn(rnd) if with_round else None, capi.DEVICE_POINTERS,
                           C.byref(info), s)
        if stream is not None:
            stream.synchronize()
        core, rnd = core.cpu().numpy(), rnd.cpu().numpy()
    else:
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        core, rnd = np.full(max(n, 1), FILL, np.int32), np.full(max(n, 1), FILL, np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.g4s_kcore(n, P(rp_h), P(ci_h if ci_h.size else core), max_k, P(core), P(rnd) if with_round else None, capi.HOST_POINTERS, C.byref(info),
                           C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        capi.check(st)
    if not with_round:
        assert np.all(rnd == FILL)                                    # a NULL round: nothing is written anywhere near
    return core[:n], (rnd[:n] if with_round else None), {k: getattr(info, k) for k, _ in capi.KCoreInfo._fields_}, st


def _check_info(info, rp, ci, n, core, levels, rounds):
    degeneracy, top = ref.top_core(core)
    assert (info["degeneracy"], info["top_core_size"], info["levels"], info["rounds"], info["capped"]) == (degeneracy, top, levels, rounds, 0), info
    assert info["edges_walked"] == int(ref.degrees(rp, ci, n).sum()), info   # every vertex is peeled once
    assert info["host_waits"] <= info["launches"] // 16 + 2 and info["scans"] <= 2 * levels, info


def _exact(rp, ci, n, core, rnd, levels, rounds, streams=(None,)):
    """both pointer kinds, round given and NULL, twice each: the reference's bits and the reference's counts"""
    infos = []
    dev = (_dev(rp), _dev(ci))
    for device in (True, False):
        for with_round in (True, False):
            for stream in streams:
                for _ in range(2):
                    a = dev if device else (rp, ci)
                    c, r, info, _ = _call(a[0], a[1], n, device=device, with_round=with_round, stream=stream)
                    assert np.array_equal(c, core), (device, with_round)
                    assert r is None or np.array_equal(r, rnd), (device, with_round)
                    _check_info(info, rp, ci, n, core, levels, rounds)
                    infos.append(info)
    return infos


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_equals_reference(name):
    n, rp, ci, core, rnd, levels, rounds = ref.case(name)
    infos = _exact(rp, ci, n, core, rnd, levels, rounds)
    print(f"{name}: {infos[0]}")


def test_the_frontier_outgrows_the_launch_grid():
    """A doubling tree deep enough for the frontier to pass eight times what the grid of its batch was sized for: the batch stops and resumes."""
    n, (rp, ci) = ref.doubling_tree(17)
    core, rnd, levels, rounds, _ = ref.kcore(rp, ci, n)
    assert rounds == 19 and int(np.bincount(rnd)[17]) == 1 << 17
    for device in (True, False):
        for _ in range(2):
            c, r, info, _ = _call(rp, ci, n, device=device)
            assert np.array_equal(c, core) and np.array_equal(r, rnd)
            _check_info(info, rp, ci, n, core, levels, rounds)
            assert info["resumes"] >= 1, info
    print(f"doubling tree of depth 17: {info}")


@pytest.fixture(scope="module")
def hubby():
    """The smallest symmetrised R-MAT of the library's own generator (edge factor 16) whose longest row passes 4096 entries: hubs in the middle of a real
    peel. (scale, CSR on the device, host arrays, the reference's results)"""
    from g4s_amd import host
    for scale in range(14, 21):
        n = 1 << scale
        A = host.csr_symmetrise(host.rmat_csr(n, scale, 16 * n, 20240613))
        rp = A.rowptr.cpu().numpy()
        if int(np.diff(rp).max()) > 4096:
            ci = A.colids.cpu().numpy()
            return scale, A, rp, ci, ref.kcore(rp, ci, n)
    raise AssertionError("no R-MAT up to scale 20 has a row above 4096 entries")


def test_larger_rmat_has_hubs_in_the_middle_of_the_peel(hubby):
    scale, A, rp, ci, (core, rnd, levels, rounds, _) = hubby
    n = A.rows
    longest = int(np.argmax(np.diff(rp)))
    assert rp[longest + 1] - rp[longest] > 4096 and rnd[longest] > 0 and levels >= 32   # a hub, appended by a crossing after many rounds of a real peel
    for device in (True, False):
        for with_round in (True, False):
            for _ in range(2):
                c, r, info, _ = _call(A.rowptr if device else rp, A.colids if device else ci, n, device=device, with_round=with_round)
                assert np.array_equal(c, core) and (r is None or np.array_equal(r, rnd))
                _check_info(info, rp, ci, n, core, levels, rounds)
    print(f"rmat{scale}: longest row {rp[longest + 1] - rp[longest]}, {info}")
    got, got_r, got_info = A.kcore(return_round=True, return_info=True)
    assert np.array_equal(got.cpu().numpy(), core) and np.array_equal(got_r.cpu().numpy(), rnd) and got_info["levels"] == levels


def test_max_k():
    import networkx as nx
    from g4s_amd import host
    n, rp, ci, core, rnd, levels, rounds = ref.case("rmat13")
    degeneracy = int(core.max())
    A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(rows[rows != ci].tolist(), ci[rows != ci].tolist()))
    for cap in (0, 1, 5, degeneracy, degeneracy + 1):
        for device in (True, False):
            for with_round in (True, False):
                for _ in range(2):
                    c, r, info, _ = _call(A.rowptr if device else rp, A.colids if device else ci, n, max_k=cap, device=device, with_round=with_round)
                    assert np.array_equal(c, np.minimum(core, cap)), cap
                    if with_round:
                        assert np.array_equal(r < 0, core >= cap) and np.all(r[r < 0] == -1) and np.array_equal(r[r >= 0], rnd[r >= 0]), cap
                    left = int(np.count_nonzero(core >= cap))
                    assert info["capped"] == int(left > 0), (cap, info)
                    if left:
                        assert (info["degeneracy"], info["top_core_size"]) == (cap, left), (cap, info)
                    assert info["levels"] == np.unique(core[core < cap]).size and info["host_waits"] <= info["launches"] // 16 + 2, (cap, info)
        c = host.kcore(A, max_k=cap)
        assert np.array_equal(c.cpu().numpy(), np.minimum(core, cap))
        sub, ids = host.kcore_subgraph(A, cap)
        want = sorted(nx.k_core(G, cap).nodes())
        assert ids.cpu().numpy().tolist() == want == np.flatnonzero(core >= cap).tolist()
        H = nx.k_core(G, cap)
        srp, sci = sub.rowptr.cpu().numpy(), sub.colids.cpu().numpy()
        relabel = np.full(n, -1, np.int64)
        relabel[want] = np.arange(len(want))
        keep = (relabel[rows] >= 0) & (relabel[ci] >= 0)                 # the induced subgraph keeps the stored diagonal entries of its vertices
        key = np.sort(relabel[rows[keep]] * len(want) + relabel[ci[keep]])
        srows = np.repeat(np.arange(len(want)), np.diff(srp))
        assert np.array_equal(np.sort(srows * len(want) + sci), key)
        off = srows != sci
        assert {(int(a), int(b)) for a, b in zip(np.asarray(want)[srows[off]], np.asarray(want)[sci[off]]) if a < b} == {(min(a, b), max(a, b)) for a, b in H.edges() if a != b}


def test_python_forms_and_empty_inputs():
    from g4s_amd import host
    n, rp, ci, core, rnd, levels, rounds = ref.case("tiny")
    A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
    assert A.kcore().cpu().numpy().tolist() == core.tolist()
    c, r = host.kcore((rp, ci), return_round=True)                    # numpy arrays: host pointers
    assert c.is_cuda and c.cpu().numpy().tolist() == core.tolist() and r.cpu().numpy().tolist() == rnd.tolist()
    c, info = host.kcore((_dev(rp), _dev(ci)), return_info=True)
    assert c.cpu().numpy().tolist() == core.tolist() and (info["degeneracy"], info["top_core_size"], info["levels"], info["rounds"]) == (2, 3, 3, 3)
    for device in (True, False):
        c, r, info, _ = _call(np.zeros(1, np.int32), np.zeros(0, np.int32), 0, device=device)       # n == 0: nothing is written
        assert c.size == 0 and info["launches"] == 0 and info["rounds"] == 0
        m = 1000
        c, r, info, _ = _call(np.zeros(m + 1, np.int32), np.zeros(0, np.int32), m, device=device)   # nnz == 0: every core 0, every round 0
        assert not c.any() and not r.any() and (info["degeneracy"], info["top_core_size"], info["levels"], info["rounds"], info["edges_walked"]) == (0, m, 1, 1, 0)
        c, r, info, _ = _call(np.array([0, 1], np.int32), np.array([0], np.int32), 1, device=device)   # one vertex with a self-loop
        assert c.tolist() == [0] and r.tolist() == [0] and info["edges_walked"] == 0


def test_degeneracy_order():
    from g4s_amd import host
    for name in ("rmat13", "hub_leaves_clique", "grid"):
        n, rp, ci, core, rnd, _, _ = ref.case(name)
        A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
        perm = host.degeneracy_order(A)
        assert perm.dtype == torch.int32 and np.array_equal(perm.cpu().numpy(), ref.degeneracy_order(rnd))
        B = host.csr_permute(A, perm)
        brp, bci = B.rowptr.cpu().numpy(), B.colids.cpu().numpy()
        rows = np.repeat(np.arange(n), np.diff(brp))
        later = np.bincount(rows[bci > rows], minlength=n)            # entries right of the diagonal: neighbours later in the order
        assert np.all(later <= core[perm.cpu().numpy()]) and later.max() <= core.max()
        assert np.all(np.bincount(rows[bci >= rows], minlength=n) <= core.max() + 1)   # at or after its own position, a stored diagonal included


def _refusal_cases():
    n, rp, ci, *_ = ref.case("grid")
    unsorted, repeated, outside, decreasing = ci.copy(), ci.copy(), ci.copy(), rp.copy()
    r = 70                                                            # an interior row: four entries
    unsorted[rp[r]], unsorted[rp[r] + 1] = ci[rp[r] + 1], ci[rp[r]]
    repeated[rp[r] + 2] = ci[rp[r] + 1]
    outside[rp[r] + 3] = n
    decreasing[r + 1] = rp[r] - 1
    return {"an unsorted row": (rp, unsorted, "ascending"), "a repeated id": (rp, repeated, "ascending"), "an id out of range": (rp, outside, "outside"),
            "a decreasing rowptr": (decreasing, ci, "rowptr")}


def test_refusals_leave_the_thread_and_stream_usable():
    """Each refusal is followed by an exact call on the same thread and stream (the recovery rule of tests/test_readback_recovery_gpu.py)."""
    from g4s_amd import capi
    lib = capi.load()
    n, rp, ci, core, rnd, levels, rounds = ref.case("grid")
    stream = torch.cuda.Stream()
    for what, (brp, bci, word) in _refusal_cases().items():
        for device in (True, False):
            _, _, _, st = _call(brp, bci, n, device=device, stream=stream, check=False)
            assert st == capi.ERR_INVALID and word in lib.g4s_last_error().decode(), (what, device, lib.g4s_last_error().decode())
            c, r, info, _ = _call(rp, ci, n, device=device, stream=stream)
            assert np.array_equal(c, core) and np.array_equal(r, rnd), (what, device)
            _check_info(info, rp, ci, n, core, levels, rounds)


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, core, rnd, *_ = ref.case("grid")
    rp_t, ci_t = _dev(rp), _dev(ci)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    out_r = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    info = capi.KCoreInfo()
    info.rounds = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_kcore(n, host._ptr(rp_t), host._ptr(ci_t), INT32_MAX, host._ptr(out), host._ptr(out_r), capi.DEVICE_POINTERS, C.byref(info),
                           C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.rounds == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(out == FILL) and torch.all(out_r == FILL)       # nothing was enqueued
    c, r, _, _ = _call(rp_t, ci_t, n, stream=stream)                 # and the library still works, on that stream too
    assert np.array_equal(c, core) and np.array_equal(r, rnd)
