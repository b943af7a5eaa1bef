"""g4s_minimum_spanning_forest on the device. Every comparison is exact: under the strict order of include/g4s.h the forest is unique, so the positions,
the labels and the pinned fields of g4s_msf_info (edges, components, weight — integer-valued weights, so the sum is exact) are compared with == against
tests/msf_ref.py (pinned to scipy and networkx in test_msf_cpu.py). Each case runs with device and with host pointers, outputs pre-filled."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import msf_ref as ref

pytestmark = pytest.mark.gpu

FILL = -7
WAITS_C = 3                                                               # include/g4s.h: host_waits <= launches / 16 + 3


def _dev(a, dt=np.int32):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dt)).cuda()   # a copy: the shared cases are read-only


def _call(rp, ci, w, n, maximum=False, device=True, stream=None, check=True, want_labels=True, flags=0):
    """The C entry point itself, outputs pre-filled: (edges array of max(n − 1, 0) with the sentinel behind info.edges, labels, info dict, status)."""
    from g4s_amd import capi, host
    lib = capi.load()
    info = capi.MSFInfo()
    flags |= capi.MSF_MAXIMUM if maximum else 0
    ne = max(n - 1, 0)
    if device:
        as_t = lambda a, dt: a if isinstance(a, torch.Tensor) else _dev(a, dt)
        rp_t, ci_t, w_t = as_t(rp, np.int32), as_t(ci, np.int32), None if w is None else as_t(w, np.float64)
        edges = torch.full((max(ne, 1),), FILL, dtype=torch.int32, device="cuda")
        labels = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())           # the arrays above were filled on the current stream
        s = C.c_void_p(stream.cuda_stream) if stream is not None else host._stream()
        st = lib.g4s_minimum_spanning_forest(n, host._ptr_nn(rp_t), host._ptr_nn(ci_t), None if w is None else host._ptr_nn(w_t), host._ptr_nn(edges),
                                             host._ptr_nn(labels) if want_labels else None, flags | capi.DEVICE_POINTERS, C.byref(info), s)
        if stream is not None:
            stream.synchronize()
        edges, labels = edges.cpu().numpy(), labels.cpu().numpy()
    else:
        spare = np.zeros(1, np.float64)
        P = lambda a: C.c_void_p(a.ctypes.data if a.size else spare.ctypes.data)
        rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        w_h = None if w is None else np.ascontiguousarray(w, np.float64)
        edges, labels = np.full(max(ne, 1), FILL, np.int32), np.full(max(n, 1), FILL, np.int32)
        st = lib.g4s_minimum_spanning_forest(n, P(rp_h), P(ci_h), None if w is None else P(w_h), P(edges), P(labels) if want_labels else None,
                                             flags | capi.HOST_POINTERS, C.byref(info), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        capi.check(st)
    return edges[:ne], labels[:n], {k: getattr(info, k) for k, _ in capi.MSFInfo._fields_}, st


def _check(got, r, n, what=None):
    edges, labels, info, _ = got
    m = r["edges"]
    assert info["edges"] == m and info["components"] == r["components"], (what, info)
    assert ref.same_weight(info["weight"], r["weight"]), (what, info, r["weight"])
    assert np.array_equal(edges[:m], r["positions"]), what
    assert (edges[m:] == FILL).all(), what                             # nothing behind info.edges is written
    assert np.array_equal(labels, r["labels"]), what
    assert info["host_waits"] <= info["launches"] // 16 + WAITS_C, info
    assert info["rounds"] <= math.ceil(math.log2(max(n, 2))) + 1, info
    assert info["resumes"] == 0 or what == "resume", info


def _exact(n, rp, ci, w, r, maximum=False, streams=(None,), what=None):
    dev = (_dev(rp), _dev(ci), _dev(w, np.float64))
    infos = []
    for device in (True, False):
        a = dev if device else (rp, ci, w)
        for stream in streams:
            got = _call(a[0], a[1], a[2], n, maximum=maximum, device=device, stream=stream)
            _check(got, r, n, (what, device))
            infos.append(got[2])
    return infos


@pytest.mark.parametrize("maximum", [False, True])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_equals_reference(name, maximum):
    n, rp, ci, w, r = ref.case(name, maximum)
    infos = _exact(n, rp, ci, w, r, maximum, what=name)
    print(f"{name} maximum={maximum}: {infos[0]}")


def test_all_ties_are_decided_by_pair_and_position():
    for name in ("grid64_null", "grid64_ones", "clique5_null", "clique5_ones"):
        n, rp, ci, w, r = ref.case(name)
        edges, labels, info, _ = _call(rp, ci, w, n)
        _check((edges, labels, info, 0), r, n, name)
        assert info["weight"] == (0.0 if w is None else float(n - 1))
    n, rp, ci, w, r = ref.case("clique5_ones")
    assert ref.pairs(rp, ci, r["positions"], n) == {(0, 1), (0, 2), (0, 3), (0, 4)}   # the smallest pairs: a star at vertex 0


def test_the_alternating_path_takes_the_most_rounds():
    rounds = {}
    for name in ("path_inc", "path_dec", "path_alt"):
        n, rp, ci, w, r = ref.case(name)
        got = _call(rp, ci, w, n)
        _check(got, r, n, name)
        rounds[name] = got[2]["rounds"]
        assert got[2]["rounds"] <= math.ceil(math.log2(n)) + 1
    print(f"rounds on the path of 5000: {rounds}")
    assert rounds["path_alt"] >= rounds["path_inc"]


def test_bridges_between_cliques_and_by_hand():
    n, rp, ci, w, r = ref.case("two_k6")
    light, heavy = (5, 11), (0, 6)
    for device in (True, False):
        got = ref.pairs(rp, ci, _call(rp, ci, w, n, device=device)[0][:n - 1], n)
        assert light in got and heavy not in got
        got = ref.pairs(rp, ci, _call(rp, ci, w, n, maximum=True, device=device)[0][:n - 1], n)
        assert heavy in got and light not in got
        edges, _, info, _ = _call(*ref.case("repeats_differ")[1:4], 4, device=device)
        assert edges.tolist() == [2, 3, 4] and info["weight"] == 10.0
        edges, _, info, _ = _call(*ref.case("repeats_equal")[1:4], 4, device=device)
        assert edges.tolist() == [0, 3, 4] and info["weight"] == 9.0
        n5, rp5, ci5, w5, r5 = ref.case("self_loops")
        edges, labels, info, _ = _call(rp5, ci5, w5, n5, device=device)
        rows = np.repeat(np.arange(n5), np.diff(rp5))
        m = info["edges"]
        assert m == 3 and (rows[edges[:m]] != ci5[edges[:m]]).all() and info["weight"] == 6.0 and labels.tolist() == [0, 0, 0, 3, 3]


def test_triangles_and_full_pattern_give_the_same_pairs():
    sets = []
    for part in ("upper", "lower", "full"):
        n, rp, ci, w, r = ref.case(f"tri_{part}")
        edges, labels, info, _ = _call(rp, ci, w, n)
        sets.append(ref.pairs(rp, ci, edges[:info["edges"]], n))
    assert sets[0] == sets[1] == sets[2]


def test_weight_values():
    inf = float("inf")
    for device in (True, False):
        # −0.0 ties with +0.0: the position decides, under both orders
        for vals in ([0.0, -0.0], [-0.0, 0.0]):
            for maximum in (False, True):
                edges, _, info, _ = _call([0, 2, 2], [1, 1], vals, 2, maximum=maximum, device=device)
                assert edges.tolist() == [0] and info["weight"] == 0.0
        # ±inf are ordinary weights: a triangle (0,1) = −inf, (1,2) = +inf, (0,2) = 5
        rp, ci, w = [0, 2, 3, 3], [1, 2, 2], [-inf, 5.0, inf]
        for maximum in (False, True):
            r = ref.forest(3, rp, ci, w, maximum)
            _check(_call(rp, ci, w, 3, maximum=maximum, device=device), r, 3, ("inf", maximum))
        assert ref.forest(3, rp, ci, w)["positions"].tolist() == [0, 1] and ref.forest(3, rp, ci, w, True)["positions"].tolist() == [1, 2]
        w2 = [inf, inf, inf]                                            # all +inf: ties again
        _check(_call(rp, ci, w2, 3, device=device), ref.forest(3, rp, ci, w2), 3, "all inf")
        n, rp, ci, w, r = ref.case("negative")
        _check(_call(rp, ci, w, n, device=device), r, n, "negative")


def test_empty_inputs_also_on_a_stream():
    for stream in (None, torch.cuda.Stream()):
        for device in (True, False):
            for w in (None, np.zeros(0)):
                edges, labels, info, _ = _call(np.zeros(1, np.int32), np.zeros(0, np.int32), w, 0, device=device, stream=stream)   # n == 0
                assert info["launches"] == 0 and info["components"] == 0 and info["edges"] == 0
                edges, labels, info, _ = _call(np.array([0, 1], np.int32), np.array([0], np.int32), None if w is None else np.ones(1), 1, device=device, stream=stream)
                assert labels.tolist() == [0] and (info["edges"], info["components"]) == (0, 1)                            # one vertex, a self-loop
                m = 1000
                edges, labels, info, _ = _call(np.zeros(m + 1, np.int32), np.zeros(0, np.int32), w, m, device=device, stream=stream)   # nnz == 0
                assert np.array_equal(labels, np.arange(m)) and (edges == FILL).all()
                assert (info["edges"], info["components"], info["weight"], info["rounds"]) == (0, m, 0.0, 0)
    edges, labels, info, _ = _call(*ref.case("two_k6")[1:4], 12, want_labels=False)                                      # labels may be NULL
    assert np.array_equal(edges, ref.case("two_k6")[4]["positions"]) and (labels == FILL).all()


def test_refusals_leave_the_thread_and_stream_usable():
    """Each refusal is followed by an exact call on the same thread and stream (the recovery rule of tests/test_readback_recovery_gpu.py)."""
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, w, r = ref.random_case(0.5, "ties")
    outside, negative, decreasing, nonzero, nan = ci.copy(), ci.copy(), rp.copy(), rp.copy(), w.copy()
    outside[ci.size // 2] = n
    negative[7] = -1
    decreasing[n // 2] = rp[n // 2 + 1] + 1
    nonzero[0] = 1
    nan[ci.size // 3] = float("nan")
    cases = {"a column id == n": (rp, outside, w, "outside"), "a negative id": (rp, negative, w, "outside"), "a decreasing rowptr": (decreasing, ci, w, "rowptr"),
             "rowptr[0] != 0": (nonzero, ci, w, "rowptr"), "a NaN": (rp, ci, nan, "NaN")}
    stream = torch.cuda.Stream()
    for what, (brp, bci, bw, word) in cases.items():
        for device in (True, False):
            _, _, _, st = _call(brp, bci, bw, n, device=device, stream=stream, check=False)
            assert st == capi.ERR_INVALID and word in lib.g4s_last_error().decode(), (what, device, lib.g4s_last_error().decode())
            _check(_call(rp, ci, w, n, device=device, stream=stream), r, n, (what, device))
    # before any HIP call: a foreign flag bit, NULLs, a negative n, overlapping outputs
    rp_t, ci_t, w_t = _dev(rp), _dev(ci), _dev(w, np.float64)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    fn, P, null, D = lib.g4s_minimum_spanning_forest, host._ptr_nn, None, capi.DEVICE_POINTERS
    refused = {
        "G4S_CC_SYMMETRIC": fn(n, P(rp_t), P(ci_t), P(w_t), P(out), null, D | capi.CC_SYMMETRIC, null, null),
        "G4S_SORT_OUTPUT": fn(n, P(rp_t), P(ci_t), P(w_t), P(out), null, D | 2, null, null),
        "rowptr": fn(n, null, P(ci_t), P(w_t), P(out), null, D, null, null),
        "edges": fn(n, P(rp_t), P(ci_t), P(w_t), null, null, D, null, null),
        "colids": fn(n, P(rp_t), null, P(w_t), P(out), null, D, null, null),
        "negative": fn(-1, P(rp_t), P(ci_t), P(w_t), P(out), null, D, null, null),
        "edges is rowptr": fn(n, P(rp_t), P(ci_t), P(w_t), P(rp_t), null, D, null, null),
        "labels is colids": fn(n, P(rp_t), P(ci_t), P(w_t), P(out), P(ci_t), D, null, null),
        "labels is edges": fn(n, P(rp_t), P(ci_t), P(w_t), P(out), P(out), D, null, null),
    }
    assert all(st == capi.ERR_INVALID for st in refused.values()), refused
    rp_h, ci_h = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    H = lambda a: C.c_void_p(a.ctypes.data)
    assert fn(n, H(rp_h), H(ci_h), null, H(ci_h[ci_h.size // 2:]), null, capi.HOST_POINTERS, null, null) == capi.ERR_INVALID   # edges inside colids
    assert "overlap" in lib.g4s_last_error().decode()
    assert (out == FILL).all()
    _check(_call(rp_t, ci_t, w_t, n), r, n, "after the refusals")


def test_a_capturing_stream_is_refused():
    from g4s_amd import capi, host
    lib = capi.load()
    n, rp, ci, w, r = ref.case("two_k6")
    rp_t, ci_t, w_t = _dev(rp), _dev(ci), _dev(w, np.float64)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    lab = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    info = capi.MSFInfo()
    info.rounds = -3
    stream = torch.cuda.Stream()
    x = torch.ones(16, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        y = x * 2.0
        st = lib.g4s_minimum_spanning_forest(n, host._ptr(rp_t), host._ptr(ci_t), host._ptr(w_t), host._ptr(out), host._ptr(lab), capi.DEVICE_POINTERS,
                                             C.byref(info), C.c_void_p(stream.cuda_stream))
        g.capture_end()
    assert st == capi.ERR_INVALID and info.rounds == -3
    assert "captur" in lib.g4s_last_error().decode()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((16,), 2.0, device="cuda"))
    assert torch.all(out == FILL) and torch.all(lab == FILL)         # nothing was enqueued
    _check(_call(rp_t, ci_t, w_t, n, stream=stream), r, n, "after the capture")   # and the library still works, on that stream too


@pytest.mark.parametrize("deg,kind", ref.RANDOM)
def test_random_graphs(deg, kind):
    """n = 50 000 at mean degree 0.5 … 4; weights out of {0 … 7} (heavy ties) or out of 2^30 (almost all distinct)."""
    from g4s_amd import host
    n, rp, ci, w, r = ref.random_case(deg, kind)
    infos = _exact(n, rp, ci, w, r, what=(deg, kind))
    cc = host.connected_components((_dev(rp), _dev(ci))).cpu().numpy()
    assert np.array_equal(r["labels"], cc)                            # the integers g4s_connected_components writes (the device labels equal r's above)
    if kind == "ties":
        _exact(n, rp, ci, None, ref.forest(n, rp, ci, None), what=(deg, "no values"))
        _exact(n, rp, ci, w, ref.forest(n, rp, ci, w, True), maximum=True, what=(deg, "maximum"))
    print(f"random deg {deg} {kind}: {infos[0]}")


def test_repeatable_on_streams_and_under_the_tuning_switches(monkeypatch):
    """Three runs, two streams, both settings of G4S_MSF_WAVE_MIN and a forced first grid: identical positions, labels and weight bits — here with
    weights that are NOT integers, so the sum's shape matters."""
    n, rp, ci, _, _ = ref.random_case(2.0, "ties")
    w = np.random.default_rng(5).uniform(-1.0, 1.0, ci.size)
    dev = (_dev(rp), _dev(ci), _dev(w, np.float64))
    r = ref.forest(n, rp, ci, w)
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    seen = []
    for env in ({}, {"G4S_MSF_WAVE_MIN": "0"}, {"G4S_MSF_FIRST_GRID": "1"}, {"G4S_MSF_FIRST_GRID": "512", "G4S_MSF_WAVE_MIN": "0"}):
        for k in ("G4S_MSF_WAVE_MIN", "G4S_MSF_FIRST_GRID"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for it in range(3):
            device = it != 2
            a = dev if device else (rp, ci, w)
            edges, labels, info, _ = _call(a[0], a[1], a[2], n, device=device, stream=streams[it % 2])
            assert np.array_equal(edges[:info["edges"]], r["positions"]) and np.array_equal(labels, r["labels"]), (env, it)
            seen.append(np.float64(info["weight"]).tobytes())
    assert len(set(seen)) == 1, seen
    assert abs(np.frombuffer(seen[0], np.float64)[0] - r["weight"]) <= 1e-9 * max(1.0, np.abs(w[r["positions"]]).sum())   # rounding of n − 1 additions, not a pinned figure


def test_launch_accounting_and_the_resume(monkeypatch):
    n, rp, ci, w, r = ref.random_case(4.0, "distinct")
    assert ci.size > 8 * 2048                                         # more entries than eight times what one workgroup is sized for
    got = _call(rp, ci, w, n)
    _check(got, r, n, "default")
    assert got[2]["resumes"] == 0
    monkeypatch.setenv("G4S_MSF_FIRST_GRID", "1")                    # the smallest grid: the live rows outgrow it at once, the batch stops and resumes
    for device in (True, False):
        got = _call(rp, ci, w, n, device=device)
        _check(got, r, n, "resume")
        assert got[2]["resumes"] > 0, got[2]
    print(f"forced resume: {got[2]}")


def test_the_forest_as_a_csr():
    from g4s_amd import host
    n, rp, ci, w, r = ref.random_case(2.0, "distinct")
    A = host.CSR(_dev(rp), _dev(ci), _dev(w, np.float64), n, n)
    positions, labels, info = A.minimum_spanning_forest(return_labels=True)
    assert np.array_equal(positions.cpu().numpy(), r["positions"]) and np.array_equal(labels.cpu().numpy(), r["labels"])
    assert {k: info[k] for k in ref.PINNED} == {k: r[k] for k in ref.PINNED}
    F = host.spanning_forest_csr(A, positions)
    assert F.nnz == 2 * info["edges"] and (F.rows, F.cols) == (n, n)
    frp, fci, fva = F.to_host()
    import scipy.sparse as sp
    S = sp.csr_matrix((fva, fci, frp), shape=(n, n))
    assert (S != S.T).nnz == 0 and S.sum() == 2 * info["weight"]
    assert torch.equal(host.connected_components(F, symmetric=True), labels)
    one_way = host.spanning_forest_csr(A, positions, symmetric=False)
    assert one_way.nnz == info["edges"]
    p2, i2 = host.minimum_spanning_forest((rp, ci, w), maximum=True)                      # numpy arrays: host pointers
    assert np.array_equal(p2.cpu().numpy(), ref.forest(n, rp, ci, w, True)["positions"])
    p3, i3 = host.minimum_spanning_forest((A.rowptr, A.colids))                            # a pair: no values
    assert i3["weight"] == 0.0 and i3["edges"] == info["edges"]
    with pytest.raises(ValueError):
        host.minimum_spanning_forest(A, maximum=1)
    with pytest.raises(ValueError):
        host.spanning_forest_csr((rp, ci), positions)
