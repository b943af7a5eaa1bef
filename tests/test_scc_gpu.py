"""g4s_strongly_connected_components on the device. Every comparison is exact: the labels are canonical and the pinned fields of g4s_scc_info are
functions of the graph under the route include/g4s.h fixes, so both are compared with == against tests/scc_ref.py (pinned to scipy and networkx in
test_scc_cpu.py). Each case runs with device and with host pointers, with the transpose given and NULL, with pre-filled outputs, twice each."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scc_ref as ref

pytestmark = pytest.mark.gpu

FILL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).cuda()            # a copy: the shared cases are read-only


def _call(rp, ci, n, tr=None, device=True, stream=None, check=True):
    """The C entry point itself, labels pre-filled: (labels, info dict, status). rp / ci / tr: numpy arrays, or device tensors with device=True."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.SCCInfo()
    if device:
        as_t = lambda a: a if isinstance(a, torch.Tensor) else _dev(a)
        rp_t, ci_t = as_t(rp), as_t(ci)
        tr_t = None if tr is None else (as_t(tr[0]), as_t(tr[1]))
        labels = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        st = lib.g4s_strongly_connected_components(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), None if tr is None else host._ptr_nn(tr_t[0]),
                                                   None if tr is None else host._ptr_nn(tr_t[1]), host._ptr_nn(labels), capi.DEVICE_POINTERS, C.byref(info), s)
        if stream is not None:
            stream.synchronize()
        labels = labels.cpu().numpy()
    else:
        spare = np.zeros(1, np.int32)
        P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        tr_h = None if tr is None else (np.ascontiguousarray(tr[0], np.int32), np.ascontiguousarray(tr[1], np.int32))
        labels = np.full(max(n, 1), FILL, np.int32)
        st = lib.g4s_strongly_connected_components(n, P(rp_h), P(ci_h), None if tr is None else P(tr_h[0]), None if tr is None else P(tr_h[1]), P(labels),
                                                   capi.HOST_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        capi.check(st)
    return labels[:n], {k: getattr(info, k) for k, _ in capi.SCCInfo._fields_}, st


def _check_info(info, r, built):
    assert {k: info[k] for k in ref.PINNED} == {k: r[k] for k in ref.PINNED}, info
    assert info["built_transpose"] == int(built), info
    assert info["host_waits"] <= info["launches"] // 16 + 5, info     # the bound include/g4s.h states


def _exact(name, streams=(None,)):
    """both pointer kinds, the transpose given and NULL, twice each: the reference's labels and the reference's counts"""
    n, rp, ci, trp, tci, r = ref.case(name)
    dev = tuple(_dev(a) for a in (rp, ci, trp, tci))
    infos = []
    for device in (True, False):
        a = dev if device else (rp, ci, trp, tci)
        for given in (True, False):
            for stream in streams:
                for _ in range(2):
                    labels, info, _ = _call(a[0], a[1], n, tr=(a[2], a[3]) if given else None, device=device, stream=stream)
                    assert np.array_equal(labels, r["labels"]), (name, device, given)
                    _check_info(info, r, not given)
                    infos.append(info)
    return infos


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_equals_reference(name):
    infos = _exact(name)
    print(f"{name}: {infos[0]}")


def test_tiny_labels_by_hand():
    n, rp, ci, *_ = ref.case("tiny")
    for device in (True, False):
        labels, info, _ = _call(rp, ci, n, device=device)
        assert labels.tolist() == ref.TINY_LABELS == [0, 1, 1, 3, 3, 3, 6, 7, 8, 9]
        assert (info["components"], info["largest"], info["largest_label"], info["trimmed"], info["pivot"], info["pivot_size"], info["color_rounds"]) == (7, 3, 3, 5, 2, 2, 1)


def test_empty_inputs_also_on_a_stream():
    for stream in (None, torch.cuda.Stream()):
        for device in (True, False):
            for given in (True, False):
                z = np.zeros(1, np.int32), np.zeros(0, np.int32)
                labels, info, _ = _call(z[0], z[1], 0, tr=z if given else None, device=device, stream=stream)    # n == 0: nothing is written
                assert labels.size == 0 and info["launches"] == 0 and info["components"] == 0 and info["pivot"] == -1
                m = 1000
                z = np.zeros(m + 1, np.int32), np.zeros(0, np.int32)
                labels, info, _ = _call(z[0], z[1], m, tr=z if given else None, device=device, stream=stream)    # nnz == 0: labels[v] = v
                assert np.array_equal(labels, np.arange(m))
                assert (info["components"], info["largest"], info["largest_label"], info["trimmed"], info["pivot"], info["color_rounds"]) == (m, 1, 0, m, -1, 0)
                assert info["built_transpose"] == int(not given)
                labels, info, _ = _call(np.array([0, 1], np.int32), np.array([0], np.int32), 1, device=device, stream=stream)   # one vertex, a self-loop
                assert labels.tolist() == [0] and info["trimmed"] == 1


def test_refusals_on_the_device_leave_the_thread_and_stream_usable():
    """Each refusal is followed by an exact call on the same thread and stream (the recovery rule of tests/test_readback_recovery_gpu.py)."""
    from g4s_amd import capi
    lib = capi.load()
    n, rp, ci, trp, tci, r = ref.case("cycles_dag")
    outside, decreasing, t_outside, t_decreasing = ci.copy(), rp.copy(), tci.copy(), trp.copy()
    outside[len(ci) // 2] = n
    decreasing[n // 2] = rp[n // 2 - 1] - 1
    t_outside[7] = -1
    t_decreasing[n // 3] = trp[n // 3 + 1] + 1
    longer = (trp.copy(), np.concatenate([tci, tci[:1]]))
    longer[0][n] += 1                                                 # a sound pattern of one more entry: trowptr[n] != rowptr[n]
    cases = {"a column id == n": (rp, outside, (trp, tci), "outside"), "a decreasing rowptr": (decreasing, ci, (trp, tci), "rowptr"),
             "a column id == n, transpose built": (rp, outside, None, "outside"), "a decreasing rowptr, transpose built": (decreasing, ci, None, "rowptr"),
             "a negative id in the transpose": (rp, ci, (trp, t_outside), "outside"), "a decreasing trowptr": (rp, ci, (t_decreasing, tci), "trowptr"),
             "trowptr[n] != rowptr[n]": (rp, ci, longer, "trowptr[n]")}
    stream = torch.cuda.Stream()
    for what, (brp, bci, btr, word) in cases.items():
        for device in (True, False):
            _, _, st = _call(brp, bci, n, tr=btr, device=device, stream=stream, check=False)
            assert st == capi.ERR_INVALID and word in lib.g4s_last_error().decode(), (what, device, lib.g4s_last_error().decode())
            labels, info, _ = _call(rp, ci, n, tr=(trp, tci), device=device, stream=stream)
            assert np.array_equal(labels, r["labels"]), (what, device)
            _check_info(info, r, False)


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, trp, tci, r = ref.case("two_cycles")
    rp_t, ci_t = _dev(rp), _dev(ci)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    info = capi.SCCInfo()
    info.trimmed = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_strongly_connected_components(n, host._ptr(rp_t), host._ptr(ci_t), None, None, host._ptr(out), capi.DEVICE_POINTERS, C.byref(info),
                                                   C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.trimmed == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(out == FILL)                                    # nothing was enqueued
    labels, _, _ = _call(rp_t, ci_t, n, stream=stream)               # and the library still works, on that stream too
    assert np.array_equal(labels, r["labels"])


def test_the_frontier_outgrows_the_launch_grid():
    """A doubling out-tree whose leaves point back to the root: one component, and a forward reach that doubles each step until it passes eight
    times what the grid of its batch was sized for: the batch stops and resumes."""
    n, rp, ci, trp, tci, r = ref.case("doubling_out_tree")
    assert r["pivot_size"] == n == (1 << 18) - 1 and r["reach_steps"][0] == 18 and not r["labels"].any()
    dev = tuple(_dev(a) for a in (rp, ci, trp, tci))
    for given in (True, False):
        for _ in range(2):
            labels, info, _ = _call(dev[0], dev[1], n, tr=dev[2:] if given else None)
            assert np.array_equal(labels, r["labels"])
            _check_info(info, r, not given)
            assert info["resumes"] >= 1, info
    labels, info, _ = _call(rp, ci, n, tr=(trp, tci), device=False)
    assert np.array_equal(labels, r["labels"]) and info["resumes"] >= 1
    print(f"doubling out-tree of depth 17: {info}")


@pytest.mark.parametrize("min_grid", ["1", "512"])
def test_the_tuning_switch_changes_nothing(min_grid, monkeypatch):
    """G4S_SCC_MIN_GRID (read at every call) moves the grids and with them where a batch stops; labels and the pinned counts stay."""
    monkeypatch.setenv("G4S_SCC_MIN_GRID", min_grid)
    for name in ("cycles_dag", "two_hubs", "doubling_out_tree"):
        n, rp, ci, trp, tci, r = ref.case(name)
        labels, info, _ = _call(rp, ci, n, tr=(trp, tci))
        assert np.array_equal(labels, r["labels"]), name
        _check_info(info, r, False)


def test_relations_to_weak_components():
    from g4s_amd import host
    n, rp, ci, trp, tci, r = ref.case("rmat13")
    A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
    S = host.csr_symmetrise(host.csr_canonical(A))                    # both directions stored: strong == weak
    wcc = host.connected_components(S)
    scc, info = host.strongly_connected_components(S, return_info=True)
    assert torch.equal(scc, wcc) and info["built_transpose"] == 1
    scc_t = S.strongly_connected_components(transpose=(S.rowptr, S.colids))   # a symmetric pattern is its own transpose
    assert torch.equal(scc_t, wcc)
    for name in ("rmat13", "cycles_dag", "two_cycles", "chain40", "er", "funnel_open"):
        n, rp, ci, trp, tci, r = ref.case(name)
        wcc = host.connected_components((_dev(rp), _dev(ci))).cpu().numpy()
        scc = host.strongly_connected_components((rp, ci), transpose=(trp, tci)).cpu().numpy()     # numpy arrays: host pointers
        assert np.array_equal(scc, r["labels"]) and np.array_equal(wcc[scc], wcc), name            # a strong component lies inside a weak one


@pytest.mark.parametrize("name", ["cycles_dag", "rmat13"])
def test_compact_labels_and_condensation(name):
    import scipy.sparse as sp
    from g4s_amd import host
    n, rp, ci, trp, tci, r = ref.case(name)
    A = host.CSR(_dev(rp), _dev(ci), torch.ones(ci.size, dtype=torch.float64, device="cuda"), n, n)
    labels = A.strongly_connected_components()
    assert np.array_equal(labels.cpu().numpy(), r["labels"])
    index, roots = host.compact_labels(labels)
    want_roots, want_index = np.unique(r["labels"], return_inverse=True)
    assert index.dtype == roots.dtype == torch.int32
    assert np.array_equal(roots.cpu().numpy(), want_roots) and np.array_equal(index.cpu().numpy(), want_index)
    Cd, index2 = host.condensation(A)
    assert torch.equal(index2, index)
    k = want_roots.size
    rows = np.repeat(np.arange(n), np.diff(rp))
    a, b = want_index[rows], want_index[ci]
    W = sp.csr_matrix((np.ones(int((a != b).sum()), np.int8), (a[a != b], b[a != b])), shape=(k, k))
    W.sum_duplicates()
    W.sort_indices()
    assert (Cd.rows, Cd.cols) == (k, k)
    assert np.array_equal(Cd.rowptr.cpu().numpy(), W.indptr) and np.array_equal(Cd.colids.cpu().numpy(), W.indices)
    own, info = Cd.strongly_connected_components(return_info=True)   # a condensation is acyclic: trimming alone finishes it
    assert np.array_equal(own.cpu().numpy(), np.arange(k)) and info["color_rounds"] == 0 and info["pivot"] == -1 and info["trimmed"] == k
    wl, winfo = host.connected_components(A, return_info=True)       # compact_labels takes the labels of either components call
    wi, wr = host.compact_labels(wl)
    u, inv = np.unique(wl.cpu().numpy(), return_inverse=True)
    assert np.array_equal(wr.cpu().numpy(), u) and np.array_equal(wi.cpu().numpy(), inv) and winfo["components"] == u.size
