"""g4s_ktruss on the device. Every comparison is exact: truss numbers, peel rounds and supports are functions of the graph alone, so they are compared
with == against tests/ktruss_ref.py (pinned to networkx.k_truss in test_ktruss_cpu.py). Each case runs with device and with host pointers, with
pre-filled outputs, with `round` / `support` given and NULL, and every call runs twice with equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ktruss_ref as ref

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
FILL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).cuda()            # a copy: the shared cases are read-only


def _call(rp, ci, n, max_k=INT32_MAX, device=True, with_round=True, with_support=True, stream=None, check=True):
    """The C entry point itself, outputs pre-filled: (truss, round or None, support or None, info dict, status)."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.KTrussInfo()
    nnz = int(ci.numel() if isinstance(ci, torch.Tensor) else np.asarray(ci).size)
    if device:
        rp_t, ci_t = (rp if isinstance(rp, torch.Tensor) else _dev(rp)), (ci if isinstance(ci, torch.Tensor) else _dev(ci))
        tr, rnd, sup = (torch.full((max(nnz, 1),), FILL, dtype=torch.int32, device="cuda") for _ in range(3))
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        st = lib.g4s_ktruss(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), max_k, host._ptr_nn(tr), host._ptr_nn(rnd) if with_round else None,
                            host._ptr_nn(sup) if with_support else None, capi.DEVICE_POINTERS, C.byref(info), s)
        if stream is not None:
            stream.synchronize()
        tr, rnd, sup = tr.cpu().numpy(), rnd.cpu().numpy(), sup.cpu().numpy()
    else:
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        tr, rnd, sup = (np.full(max(nnz, 1), FILL, np.int32) for _ in range(3))
        P = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.g4s_ktruss(n, P(rp_h), P(ci_h if ci_h.size else tr), max_k, P(tr), P(rnd) if with_round else None, P(sup) if with_support else None,
                            capi.HOST_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        capi.check(st)
    if not with_round:
        assert np.all(rnd == FILL)                                    # a NULL output: nothing is written anywhere near
    if not with_support:
        assert np.all(sup == FILL)
    assert np.all(tr[nnz:] == FILL) and np.all(rnd[nnz:] == FILL) and np.all(sup[nnz:] == FILL)
    return (tr[:nnz], rnd[:nnz] if with_round else None, sup[:nnz] if with_support else None,
            {k: getattr(info, k) for k, _ in capi.KTrussInfo._fields_}, st)


def _check_info(info, rp, ci, n, support, truss, levels, rounds):
    m, triangles, top, top_edges = ref.facts(rp, ci, n, support, truss)
    got = (info["triangles"], info["max_truss"], info["top_truss_edges"], info["levels"], info["rounds"], info["capped"])
    assert got == (triangles, top, top_edges, levels, rounds, 0), info
    _, eu, ev = ref.edge_ids(rp, ci, n)
    bound = int(ref.walk_len(rp, eu, ev).sum())                       # every edge is peeled once, along its shorter row
    assert 0 <= info["edges_walked"] <= bound and info["support_walked"] == bound, (info, bound)
    assert info["host_waits"] <= info["launches"] // 16 + 2 and info["scans"] <= 2 * levels, info


def _exact(name, streams=(None,)):
    """both pointer kinds, round / support given and NULL, twice each: the reference's bits and the reference's counts"""
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case(name)
    infos = []
    dev = (_dev(rp), _dev(ci))
    for device in (True, False):
        for with_round, with_support in ((True, True), (False, True), (True, False), (False, False)):
            for stream in streams:
                for _ in range(2):
                    a = dev if device else (rp, ci)
                    t, r, s, info, _ = _call(a[0], a[1], n, device=device, with_round=with_round, with_support=with_support, stream=stream)
                    assert np.array_equal(t, truss), (device, with_round, with_support)
                    assert r is None or np.array_equal(r, rnd), (device, with_round, with_support)
                    assert s is None or np.array_equal(s, support), (device, with_round, with_support)
                    _check_info(info, rp, ci, n, support, truss, levels, rounds)
                    infos.append(info)
    return infos


def _csr(rp, ci, n):
    from g4s_amd import host
    return host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)


@pytest.mark.parametrize("name", [c for c in ref.CASES if c != "tri_tree"])
def test_case_equals_reference(name):
    from g4s_amd import host
    infos = _exact(name)
    print(f"{name}: {infos[0]}")
    n, rp, ci, *_ = ref.case(name)
    assert infos[0]["triangles"] == host.triangle_count(_csr(rp, ci, n))


def test_the_frontier_outgrows_the_launch_grid():
    """tri_tree: a peel builds a frontier with more walk entries than eight times what the grid of its batch was sized for (the property is asserted
    from the reference in test_ktruss_cpu.py): the batch stops and resumes."""
    from g4s_amd import host
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case("tri_tree")
    dev = (_dev(rp), _dev(ci))
    for device in (True, False):
        for _ in range(2):
            a = dev if device else (rp, ci)
            t, r, s, info, _ = _call(a[0], a[1], n, device=device)
            assert np.array_equal(t, truss) and np.array_equal(r, rnd) and np.array_equal(s, support)
            _check_info(info, rp, ci, n, support, truss, levels, rounds)
            assert info["resumes"] >= 1, info
    print(f"tri_tree: {info}")
    assert info["triangles"] == host.triangle_count(_csr(rp, ci, n))


def test_support_equals_the_masked_product():
    from g4s_amd import host
    n, rp, ci, support, truss, rnd, _, _ = ref.case("rmat11")
    A = _csr(rp, ci, n)
    A0 = host.csr_select(A, "offdiag")                                # a stored diagonal entry would add walks through the loop to A·A
    Cm = host.spgemm_masked(A0, A0, A0, pattern_only=True)
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = ci != rows
    assert np.array_equal(A0.colids.cpu().numpy(), ci[off])
    got = host.ktruss(A, return_support=True)[1].cpu().numpy()
    assert np.array_equal(got, support) and np.array_equal(got[off], Cm.values.cpu().numpy().astype(np.int64)) and not got[~off].any()


def test_max_k():
    import networkx as nx
    from g4s_amd import host
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case("rmat10")
    top = int(truss.max())
    A = _csr(rp, ci, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    off, up = ci != rows, ci > rows
    G = ref.networkx_graph(rp, ci, n)
    for cap in (2, 3, 5, top, top + 1):
        left = int(np.count_nonzero(up & (truss >= cap)))
        for device in (True, False):
            for with_round in (True, False):
                for _ in range(2):
                    t, r, s, info, _ = _call(A.rowptr if device else rp, A.colids if device else ci, n, max_k=cap, device=device, with_round=with_round)
                    assert np.array_equal(t, np.minimum(truss, cap)) and np.array_equal(s, support), cap
                    if with_round:
                        assert np.array_equal(r[off] < 0, truss[off] >= cap) and np.all(r[r < 0] == -1) and np.array_equal(r[r >= 0], rnd[r >= 0]), cap
                    assert info["capped"] == int(left > 0), (cap, info)
                    if left:
                        assert (info["max_truss"], info["top_truss_edges"]) == (cap, left), (cap, info)
                    assert info["levels"] == np.unique(truss[off & (truss < cap)]).size and info["host_waits"] <= info["launches"] // 16 + 2, (cap, info)
        t = host.ktruss(A, max_k=cap)
        assert np.array_equal(t.cpu().numpy(), np.minimum(truss, cap))
        sub = host.ktruss_subgraph(A, cap)
        assert (sub.rows, sub.cols) == (n, n)
        srp, sci = sub.rowptr.cpu().numpy(), sub.colids.cpu().numpy()
        srows = np.repeat(np.arange(n), np.diff(srp))
        assert np.all(sub.values.cpu().numpy() == cap)
        want = {(min(a, b), max(a, b)) for a, b in nx.k_truss(G, cap).edges()}
        assert {(int(a), int(b)) for a, b in zip(srows, sci) if a < b} == want == {(int(b), int(a)) for a, b in zip(srows, sci) if a > b}


def test_python_forms_and_empty_inputs():
    from g4s_amd import host
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case("k4_ear")
    A = _csr(rp, ci, n)
    assert A.ktruss().cpu().numpy().tolist() == truss.tolist()
    t, r = host.ktruss((rp, ci), return_round=True)                   # numpy arrays: host pointers
    assert t.is_cuda and t.cpu().numpy().tolist() == truss.tolist() and r.cpu().numpy().tolist() == rnd.tolist()
    t, s, info = host.ktruss((_dev(rp), _dev(ci)), return_support=True, return_info=True)
    assert t.cpu().numpy().tolist() == truss.tolist() and s.cpu().numpy().tolist() == support.tolist()
    assert (info["triangles"], info["max_truss"], info["top_truss_edges"], info["levels"], info["rounds"]) == (5, 4, 6, 2, 2)
    t, r, s = A.ktruss(max_k=4, return_round=True, return_support=True)
    assert t.cpu().numpy().tolist() == truss.tolist() and r.cpu().numpy().tolist() == np.where(truss == 4, -1, rnd).tolist()
    for device in (True, False):
        t, r, s, info, _ = _call(np.zeros(1, np.int32), np.zeros(0, np.int32), 0, device=device)          # n == 0: nothing is written
        assert t.size == 0 and info["launches"] == 0 and info["rounds"] == 0
        m = 1000
        t, r, s, info, _ = _call(np.zeros(m + 1, np.int32), np.zeros(0, np.int32), m, device=device)      # nnz == 0: nothing to write either
        assert t.size == 0 and (info["triangles"], info["max_truss"], info["top_truss_edges"], info["levels"], info["rounds"], info["capped"]) == (0,) * 6
        t, r, s, info, _ = _call(np.array([0, 1], np.int32), np.array([0], np.int32), 1, device=device)   # one vertex with a self-loop
        assert (t.tolist(), r.tolist(), s.tolist()) == ([0], [-1], [0])
        assert (info["triangles"], info["max_truss"], info["levels"], info["rounds"], info["edges_walked"], info["capped"]) == (0,) * 6


def _refusal_cases():
    n, rp, ci, *_ = ref.case("tri_grid")
    unsorted, repeated, outside, decreasing = ci.copy(), ci.copy(), ci.copy(), rp.copy()
    r = 70                                                            # an interior row: six entries
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
    n, rp, ci, support, truss, rnd, levels, rounds = ref.case("tri_grid")
    stream = torch.cuda.Stream()
    for what, (brp, bci, word) in _refusal_cases().items():
        for device in (True, False):
            *_, st = _call(brp, bci, n, device=device, stream=stream, check=False)
            assert st == capi.ERR_INVALID and word in lib.g4s_last_error().decode(), (what, device, lib.g4s_last_error().decode())
            t, r, s, info, _ = _call(rp, ci, n, device=device, stream=stream)
            assert np.array_equal(t, truss) and np.array_equal(r, rnd) and np.array_equal(s, support), (what, device)
            _check_info(info, rp, ci, n, support, truss, levels, rounds)


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, support, truss, rnd, *_ = ref.case("tri_grid")
    rp_t, ci_t = _dev(rp), _dev(ci)
    outs = [torch.full((ci.size,), FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    info = capi.KTrussInfo()
    info.rounds = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_ktruss(n, host._ptr(rp_t), host._ptr(ci_t), INT32_MAX, host._ptr(outs[0]), host._ptr(outs[1]), host._ptr(outs[2]),
                            capi.DEVICE_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.rounds == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert all(bool(torch.all(o == FILL)) for o in outs)             # nothing was enqueued
    t, r, s, _, _ = _call(rp_t, ci_t, n, stream=stream)              # and the library still works, on that stream too
    assert np.array_equal(t, truss) and np.array_equal(r, rnd) and np.array_equal(s, support)
