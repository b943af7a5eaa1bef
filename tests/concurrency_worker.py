"""The program behind tests/test_concurrency_gpu.py: `python tests/concurrency_worker.py <scenario>` runs ONE scenario of concurrent use of
libg4s_hip.so on cuda:0 and prints one JSON line: {"scenario", "calls", "n_differences", "differences" (the first 20), "serial_s", "concurrent_s",
"total_s"}. The test asserts that nothing differed. Every comparison is == against tests/concurrency_cases.py (integer values: exact in any order).

Each scenario first runs its work serially (one call at a time, the same calls on the same streams — also the source of the info fields the
concurrent run is compared with), then concurrently: a fixed 8 rounds, at most 6 host threads (never sized by the CPU count), each thread under its
own torch.cuda.Stream; ctypes releases the GIL during a call. Order between threads, where a scenario needs one, comes from threading.Barrier.
A thread that raises aborts the barriers, so the others end too; the exception is reported as a difference."""
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from g4s_amd import capi, host
from tests import concurrency_cases as cc

SCENARIOS = ("handles_on_streams", "threads_synchronous_calls", "carried_product", "carried_trim", "carried_symbolic", "carried_inplace",
             "errors_stay_with_their_thread")
SR = host.SEMIRINGS
DEV = capi.DEVICE_POINTERS
BARRIER_TIMEOUT = cc.BARRIER_TIMEOUT   # a barrier nobody else reaches ends the scenario with a difference, before the child's time limit

lib = None
_lock = threading.Lock()
differences = []
calls = [0]
_own = threading.local()          # .n: the differences THIS thread recorded


def differ(what):
    _own.n = own_differences() + 1
    with _lock:
        differences.append(what)


def own_differences():
    return getattr(_own, "n", 0)


def called(n=1):
    with _lock:
        calls[0] += n


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return differ(f"{what}: shape {got.shape} != {want.shape}")
    bad = np.flatnonzero((got != want).ravel())
    if bad.size:
        differ(f"{what}: {bad.size} of {got.size} differ, first at {int(bad[0])}: {got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}")


def same_values(what, got, want):
    same(what, np.asarray(got) + 0.0, np.asarray(want) + 0.0)     # −0 == +0: the sign of a zero is outside the contract


def ok(what, status):
    if status != capi.OK:
        differ(f"{what}: status {status}: {lib.g4s_last_error().decode()}")
    return status == capi.OK


def dptr(t):
    return C.c_void_p(t.data_ptr())


def hptr(a):
    return C.c_void_p(a.ctypes.data)


def cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def prepare(P):
    """every expected result the scenarios look up, computed before anything is timed (they are cached on the Product)"""
    for s in cc.SEMIRINGS:
        P.cval(s)
        P.cval(s, True)
        P.masked(s)
    P.masked("plus_times", True)
    _ = P.masked_products, P.triangles, P.labels, P.cc_stats, P.transpose, P.spmv, P.sssp, P.bfs


class Dev:
    """a Product's arrays on the device (shared by the threads: inputs are only read), uploaded and complete before any thread starts"""

    def __init__(self, P):
        self.P = P
        self.rp, self.ci, self.va, self.va2 = up(P.A[0]), up(P.A[1]), up(P.A[2]), up(P.A2[2])
        self.grp, self.gci = up(P.graph[0]), up(P.graph[1])
        self.x, self.y0 = up(P.x), up(P.y0)


# ------------------------------------------------------------------------------------------------ one call each, compared on the spot
serial_info = {}                  # (op, problem, variant) -> info fields of the serial run
_serial_pass = [True]


def info_same(key, fields):
    if _serial_pass[0]:
        serial_info.setdefault(key, fields)
    if serial_info.get(key) != fields:
        differ(f"{key}: info {fields} != serial {serial_info.get(key)}")


def op_onecall_dev(d, semiring):
    P = d.P
    crpt, ccol, cval, cnnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
    st = lib.g4s_spgemm_csr_i32_f64(dptr(d.rp), dptr(d.ci), dptr(d.va), dptr(d.rp), dptr(d.ci), dptr(d.va), C.byref(crpt), C.byref(ccol), C.byref(cval),
                                    P.n, P.n, P.n, C.byref(cnnz), None, DEV | capi.SORT_OUTPUT | SR[semiring])
    called()
    what = f"onecall_dev {P.name} {semiring}"
    if ok(what, st):
        same(what + " cnnz", cnnz.value, P.cnnz)
        if cnnz.value == P.cnnz:
            same(what + " crpt", host.view_i32(crpt, P.n + 1).cpu().numpy(), P.crpt)
            same(what + " ccol", host.view_i32(ccol, P.cnnz).cpu().numpy(), P.ccol)
            same_values(what + " cval", host.view_f64(cval, P.cnnz).cpu().numpy(), P.cval(semiring))
    for p in (crpt, ccol, cval):                                   # back to the cache while other threads allocate
        if p.value:
            lib.g4s_dev_free(p)


def op_onecall_host(d, semiring):
    P = d.P
    crpt, ccol, cval, cnnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
    st = lib.g4s_spgemm_csr_i32_f64(hptr(P.A[0]), hptr(P.A[1]), hptr(P.A[2]), hptr(P.A[0]), hptr(P.A[1]), hptr(P.A[2]), C.byref(crpt), C.byref(ccol),
                                    C.byref(cval), P.n, P.n, P.n, C.byref(cnnz), None, capi.HOST_POINTERS | capi.SORT_OUTPUT | SR[semiring])
    called()
    what = f"onecall_host {P.name} {semiring}"
    if ok(what, st):
        same(what + " cnnz", cnnz.value, P.cnnz)
        if cnnz.value == P.cnnz:
            same(what + " crpt", np.ctypeslib.as_array(C.cast(crpt, capi.i32p), (P.n + 1,)), P.crpt)
            same(what + " ccol", np.ctypeslib.as_array(C.cast(ccol, capi.i32p), (P.cnnz,)), P.ccol)
            same_values(what + " cval", np.ctypeslib.as_array(C.cast(cval, capi.f64p), (P.cnnz,)), P.cval(semiring))
    for p in (crpt, ccol, cval):
        lib.g4s_free(p)


def symbolic(d, crpt, what):
    P, cnnz = d.P, C.c_int64(0)
    st = lib.g4s_spgemm_symbolic(P.n, P.n, P.n, dptr(d.rp), dptr(d.ci), dptr(d.rp), dptr(d.ci), dptr(crpt), C.byref(cnnz), cur())
    called()
    if ok(what + " symbolic", st):
        same(what + " cnnz", cnnz.value, P.cnnz)
        return cnnz.value == P.cnnz
    return False


def numeric(d, crpt, semiring, what, va=None, second=False):
    P = d.P
    va = d.va if va is None else va
    ccol = torch.empty(P.cnnz, dtype=torch.int32, device="cuda")
    cval = torch.empty(P.cnnz, dtype=torch.float64, device="cuda")
    st = lib.g4s_spgemm_numeric(P.n, P.n, P.n, dptr(d.rp), dptr(d.ci), dptr(va), dptr(d.rp), dptr(d.ci), dptr(va), dptr(crpt), dptr(ccol), dptr(cval),
                                DEV | capi.SORT_OUTPUT | SR[semiring], cur())
    called()
    if ok(what + " numeric", st):
        same(what + " crpt", crpt.cpu().numpy(), P.crpt)
        same(what + " ccol", ccol.cpu().numpy(), P.ccol)
        same_values(what + " cval", cval.cpu().numpy(), P.cval(semiring, second))


def op_two_call(d, semiring):
    what = f"two_call {d.P.name} {semiring}"
    crpt = torch.empty(d.P.n + 1, dtype=torch.int32, device="cuda")
    if symbolic(d, crpt, what):
        numeric(d, crpt, semiring, what)


def op_masked(d, semiring, pattern_only=False):
    P = d.P
    cval = torch.empty(P.nnz, dtype=torch.float64, device="cuda")
    info, null = capi.MaskedInfo(), C.c_void_p(0)
    st = lib.g4s_spgemm_masked(P.n, P.n, P.n, dptr(d.rp), dptr(d.ci), null if pattern_only else dptr(d.va), dptr(d.rp), dptr(d.ci),
                               null if pattern_only else dptr(d.va), dptr(d.rp), dptr(d.ci), dptr(cval), DEV | SR[semiring], C.byref(info), cur())
    called()
    what = f"masked {P.name} {semiring}{' pattern' if pattern_only else ''}"
    if ok(what, st):
        same_values(what + " cval", cval.cpu().numpy(), P.masked(semiring, pattern_only))
        same(what + " mask_nnz", info.mask_nnz, P.nnz)
        same(what + " products", info.products, P.masked_products)
        info_same(("masked", P.name), (info.mask_nnz, info.products, info.rows_wave, info.rows_lds, info.rows_global, info.rows_split))


def op_triangles(d):
    P, count, info = d.P, C.c_int64(0), capi.MaskedInfo()
    st = lib.g4s_triangle_count(P.n, dptr(d.grp), dptr(d.gci), C.byref(count), DEV, C.byref(info), cur())
    called()
    what = f"triangles {P.name}"
    if ok(what, st):
        same(what, count.value, P.triangles)
        info_same(("triangles", P.name), (info.mask_nnz, info.products, info.rows_wave, info.rows_lds, info.rows_global, info.rows_split))


def op_components(d, on_host):
    P, info = d.P, capi.CCInfo()
    if on_host:
        lab = np.empty(P.n, np.int32)
        st = lib.g4s_connected_components(P.n, hptr(P.A[0]), hptr(P.A[1]), hptr(lab), capi.HOST_POINTERS, C.byref(info), cur())
    else:
        out = torch.empty(P.n, dtype=torch.int32, device="cuda")
        st = lib.g4s_connected_components(P.n, dptr(d.rp), dptr(d.ci), dptr(out), DEV, C.byref(info), cur())
    called()
    what = f"components {P.name} {'host' if on_host else 'device'}"
    if ok(what, st):
        same(what + " labels", lab if on_host else out.cpu().numpy(), P.labels)
        same(what + " (components, largest, largest_label)", (info.components, info.largest, info.largest_label), P.cc_stats)
        info_same(("components", P.name), (info.components, info.largest, info.largest_label, info.sample_rounds))


def op_transpose(d):
    P = d.P
    trp = torch.empty(P.n + 1, dtype=torch.int32, device="cuda")
    tci, perm = (torch.empty(P.nnz, dtype=torch.int32, device="cuda") for _ in range(2))
    tva = torch.empty(P.nnz, dtype=torch.float64, device="cuda")
    st = lib.g4s_csr_transpose(P.n, P.n, P.nnz, dptr(d.rp), dptr(d.ci), dptr(d.va), dptr(trp), dptr(tci), dptr(tva), dptr(perm), DEV, cur())
    called()
    what = f"transpose {P.name}"
    if ok(what, st):
        for name, got, want in zip(("trowptr", "tcolids", "tvalues", "perm"), (trp, tci, tva, perm), P.transpose):
            same(f"{what} {name}", got.cpu().numpy(), want)


def op_spmv_host(d):
    P = d.P
    y = P.y0.copy()
    st = lib.g4s_spmv_csr_i32_f64(P.n, P.n, hptr(P.A[0]), hptr(P.A[1]), hptr(P.A[2]), hptr(P.x), hptr(y), 2.0, -3.0, capi.HOST_POINTERS)
    called()
    if ok(f"spmv_host {P.name}", st):
        same(f"spmv_host {P.name}", y, P.spmv)


def op_create_destroy_blocked(d):
    """a blocked-path handle made from host arrays, one product on the thread's stream, destroyed again"""
    P, h, info = d.P, C.c_void_p(), capi.CsrInfo()
    what = f"create_destroy_blocked {P.name}"
    if not ok(what + " create", lib.g4s_csr_create(C.byref(h), P.n, P.n, P.nnz, hptr(P.A[0]), hptr(P.A[1]), hptr(P.A[2]), capi.HOST_POINTERS | capi.SPMV_BLOCKED)):
        return
    y = d.y0.clone()
    if ok(what + " info", lib.g4s_csr_get_info(h, C.byref(info))):
        same(what + " spmv_path", info.spmv_path, 1)
        info_same(("blocked_plan", P.name), (info.rows, info.cols, info.nnz, info.spmv_path))
    if ok(what + " spmv", lib.g4s_spmv(h, dptr(d.x), dptr(y), 2.0, -3.0, cur())):
        torch.cuda.current_stream().synchronize()
        same(what + " y", y.cpu().numpy(), P.spmv)
    called(3)
    ok(what + " destroy", lib.g4s_csr_destroy(h))


class Traversal:
    """the two handles a thread owns: the weighted graph (g4s_sssp) and A itself with its stored zeros (g4s_bfs)"""

    def __init__(self, P):
        self.P = P
        W, self.src = P.weights
        self.w = host.CSR.from_host(*W, P.n, P.n)
        self.a = host.CSR.from_host(*P.A, P.n, P.n)
        self.w.traverse_reserve()
        self.a.traverse_reserve()

    def sssp(self):
        P, info = self.P, capi.TraverseInfo()
        dist = torch.empty(P.n, dtype=torch.float64, device="cuda")
        src = np.array([self.src], np.int32)
        st = lib.g4s_sssp(self.w.handle, hptr(src), 1, dptr(dist), 0, 0, C.byref(info), cur())
        called()
        if ok(f"sssp {P.name}", st):
            same_values(f"sssp {P.name}", dist.cpu().numpy(), P.sssp)
            same(f"sssp {P.name} (reached, converged)", (info.reached, info.converged), (int(np.isfinite(P.sssp).sum()), 1))

    def bfs(self):
        P, info = self.P, capi.TraverseInfo()
        level = torch.empty(P.n, dtype=torch.int32, device="cuda")
        src = np.array([self.src], np.int32)
        st = lib.g4s_bfs(self.a.handle, hptr(src), 1, dptr(level), 0, 0, C.byref(info), cur())
        called()
        if ok(f"bfs {P.name}", st):
            same(f"bfs {P.name}", level.cpu().numpy(), P.bfs)
            same(f"bfs {P.name} (reached, converged)", (info.reached, info.converged), (int((P.bfs >= 0).sum()), 1))


# the calls of scenario b: (name, function of (thread context, Dev))
OPS = (
    ("onecall_dev plus_times", lambda t, d: op_onecall_dev(d, "plus_times")),
    ("masked min_plus", lambda t, d: op_masked(d, "min_plus")),
    ("components device", lambda t, d: op_components(d, False)),
    ("two_call plus_times", lambda t, d: op_two_call(d, "plus_times")),
    ("sssp", lambda t, d: t.traversal.sssp()),
    ("onecall_host min_plus", lambda t, d: op_onecall_host(d, "min_plus")),
    ("masked plus_times", lambda t, d: op_masked(d, "plus_times")),
    ("transpose", lambda t, d: op_transpose(d)),
    ("triangles", lambda t, d: op_triangles(d)),
    ("onecall_dev min_plus", lambda t, d: op_onecall_dev(d, "min_plus")),
    ("masked or_and", lambda t, d: op_masked(d, "or_and")),
    ("spmv_host", lambda t, d: op_spmv_host(d)),
    ("two_call max_plus", lambda t, d: op_two_call(d, "max_plus")),
    ("components host", lambda t, d: op_components(d, True)),
    ("masked plus_times pattern", lambda t, d: op_masked(d, "plus_times", True)),
    ("bfs", lambda t, d: t.traversal.bfs()),
    ("masked max_plus", lambda t, d: op_masked(d, "max_plus")),
    ("create_destroy_blocked", lambda t, d: op_create_destroy_blocked(d)),
    ("onecall_host plus_times", lambda t, d: op_onecall_host(d, "plus_times")),
)
assert tuple(name for name, _ in OPS) == cc.OP_NAMES


class ThreadCtx:
    def __init__(self, index):
        self.index = index
        self.stream = torch.cuda.Stream()
        self.traversal = None


def run_threads(bodies, barriers=()):
    """one host thread per body; an exception in one aborts the barriers so that nobody waits for it"""
    def guard(body):
        try:
            body()
        except threading.BrokenBarrierError:
            differ("a barrier was broken: another thread ended early")
        except Exception as e:  # noqa: BLE001  (reported, not swallowed: the scenario fails)
            differ(f"exception: {type(e).__name__}: {e}")
            for b in barriers:
                b.abort()
    threads = [threading.Thread(target=guard, args=(b,)) for b in bodies]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


def lockstep(ctxs, slots, concurrent):
    """slots: a list of {thread index: function}; the functions of one slot run at the same time, slot after slot (threading.Barrier between them) —
    or, serially, one after the other in the main thread. Every function runs under its thread's stream."""
    def run(i, fn):
        with torch.cuda.stream(ctxs[i].stream):
            fn()
            torch.cuda.current_stream().synchronize()
    if not concurrent:
        for slot in slots:
            for i in sorted(slot):
                run(i, slot[i])
        return
    barrier = threading.Barrier(len(ctxs), timeout=BARRIER_TIMEOUT)

    def body(i):
        def f():
            for slot in slots:
                barrier.wait()
                if i in slot:
                    run(i, slot[i])
        return f
    run_threads([body(i) for i in range(len(ctxs))], (barrier,))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------ a. handles_on_streams
def handles_on_streams():
    flags = {"stream": capi.SPMV_STREAM, "blocked": capi.SPMV_BLOCKED, "diagonal": 0, "block_row": 0}
    hs, streams = [], []
    for H in cc.handles():
        A = host.CSR.from_host(*H.A, H.n, H.n, spmv_flags=flags[H.path])
        same(f"{H.path}: spmv_path", A.info()["spmv_path"], cc.SPMV_PATHS[H.path])
        A.transpose_reserve()
        A.spmm_reserve(H.K)
        hs.append(A)
        streams.append(torch.cuda.Stream())
    calls_of = ("spmv", "spmm", "min_plus_acc", "transpose")

    def buffers():
        """fresh inputs and outputs for every (round, handle), complete before anything is enqueued"""
        out = {}
        for r in range(cc.ROUNDS):
            for i, H in enumerate(cc.handles()):
                inp = H.inputs(r)
                out[r, i] = {"x": up(inp["x"]), "X": up(inp["X"]), "xt": up(inp["xt"]), "spmv": torch.full((H.n,), float("nan"), dtype=torch.float64, device="cuda"),
                             "spmm": torch.full((H.n, H.K), float("nan"), dtype=torch.float64, device="cuda"), "min_plus_acc": up(inp["y_acc"]),
                             "transpose": torch.full((H.n,), float("nan"), dtype=torch.float64, device="cuda")}
        torch.cuda.synchronize()
        return out

    def enqueue(which, A, b, s):
        sp = C.c_void_p(s.cuda_stream)
        h = A.handle
        if which == "spmv":
            st = lib.g4s_spmv(h, dptr(b["x"]), dptr(b["spmv"]), 1.0, 0.0, sp)
        elif which == "spmm":
            st = lib.g4s_spmm(h, A_K, dptr(b["X"]), A_K, dptr(b["spmm"]), A_K, 1.0, 0.0, 0, sp)
        elif which == "min_plus_acc":
            st = lib.g4s_spmv_semiring(h, dptr(b["x"]), dptr(b["min_plus_acc"]), capi.SEMIRING_MIN_PLUS | capi.SPMV_ACCUMULATE, sp)
        else:
            st = lib.g4s_spmv_transpose(h, dptr(b["xt"]), dptr(b["transpose"]), 1.0, 0.0, sp)
        called()
        ok(which, st)

    A_K = cc.Handle.K
    alone = buffers()

    def serial():                                                   # every call alone: enqueued, then waited for
        for r in range(cc.ROUNDS):
            for i, A in enumerate(hs):
                for which in calls_of:
                    enqueue(which, A, alone[r, i], streams[i])
                    streams[i].synchronize()
    t_serial = timed(serial)
    mixed = buffers()

    def concurrent():                                               # round-robin over the handles, nothing waited for until the end
        for r in range(cc.ROUNDS):
            for which in calls_of:
                for i, A in enumerate(hs):
                    enqueue(which, A, mixed[r, i], streams[i])
    t_conc = timed(concurrent)
    for r in range(cc.ROUNDS):
        for i, H in enumerate(cc.handles()):
            want = H.expected(r)
            for which in calls_of:
                a, m = alone[r, i][which].cpu().numpy(), mixed[r, i][which].cpu().numpy()
                same_values(f"{H.path} round {r} {which}: alone against the reference", a, want[which])
                same_values(f"{H.path} round {r} {which}: interleaved against the reference", m, want[which])
                same(f"{H.path} round {r} {which}: interleaved against alone", m.view(np.int64), a.view(np.int64))
    for A in hs:
        A.close()
    return t_serial, t_conc


# ------------------------------------------------------------------------------------------------ b. threads_synchronous_calls
def threads_synchronous_calls():
    for P in cc.products():
        prepare(P)
    devs = [Dev(P) for P in cc.products()]
    ctxs = [ThreadCtx(i) for i in range(cc.THREADS)]
    for t in ctxs:
        t.traversal = Traversal(cc.products()[t.index % 3])         # handles of its own: each of the three problems is owned by two threads
    torch.cuda.synchronize()
    TRIMMER = 3                                                     # the thread that also calls g4s_trim, in the middle of each of its rounds

    pair = threading.Barrier(2, timeout=BARRIER_TIMEOUT)

    def body(t, concurrent):
        def f():
            with torch.cuda.stream(ctxs[t].stream):
                for r, round_jobs in enumerate(cc.schedule(t)):
                    if t < 2:                                       # the same large-enough product in two threads at once: one of them finds the column scratch taken
                        if concurrent:
                            pair.wait()
                        op_onecall_dev(devs[2], "plus_times" if r % 2 == 0 else "min_plus")
                    for j, (op, p) in enumerate(round_jobs):
                        if t == TRIMMER and j == 2:                 # beside whatever the other five are in: cached blocks, the carried state, the column scratch
                            called()
                            ok("g4s_trim", lib.g4s_trim())
                        OPS[op][1](ctxs[t], devs[p])
                torch.cuda.current_stream().synchronize()
        return f

    def serial():
        for t in range(cc.THREADS):
            body(t, False)()
    t_serial = timed(serial)
    _serial_pass[0] = False
    t_conc = timed(lambda: run_threads([body(t, True) for t in range(cc.THREADS)], (pair,)))
    return t_serial, t_conc


# ------------------------------------------------------------------------------------------------ c. carried_symbolic_interleaved
def carried(variant):
    P1, P2 = cc.products()[0], cc.products()[1]
    prepare(P1); prepare(P2)
    d1, d2 = Dev(P1), Dev(P2)
    ctxs = [ThreadCtx(0), ThreadCtx(1)]
    crpt1 = torch.empty(P1.n + 1, dtype=torch.int32, device="cuda")   # the same buffers every round: the carried state is keyed by the pointers
    crpt2 = torch.empty(P2.n + 1, dtype=torch.int32, device="cuda")
    values = torch.empty_like(d1.va)
    torch.cuda.synchronize()
    state = {}

    def slots():
        out = []
        for r in range(cc.ROUNDS):
            sem = ("plus_times", "min_plus", "max_plus", "or_and")[r % 4]

            def a1():
                values.copy_(d1.va)
                state["ok"] = symbolic(d1, crpt1, f"A round {r}")

            def b2():
                if variant == "product":
                    op_onecall_dev(d2, sem)
                elif variant == "trim":
                    called()
                    ok("g4s_trim", lib.g4s_trim())
                else:
                    state["ok2"] = symbolic(d2, crpt2, f"B round {r}")

            def a3():
                if state["ok"]:
                    numeric(d1, crpt1, sem, f"A round {r} first", va=values)

            def b3():
                if state.get("ok2"):
                    numeric(d2, crpt2, sem, f"B round {r}")

            def a4():
                if state["ok"]:
                    values.copy_(d1.va2)                            # new integer values, same pattern, same buffer
                    numeric(d1, crpt1, "plus_times" if r % 2 == 0 else sem, f"A round {r} second", va=values, second=True)
            out += [{0: a1}, {1: b2}, {0: a3, 1: b3} if variant == "symbolic" else {0: a3}, {0: a4}]
        return out

    t_serial = timed(lambda: lockstep(ctxs, slots(), False))
    t_conc = timed(lambda: lockstep(ctxs, slots(), True))
    ok("g4s_trim", lib.g4s_trim())
    return t_serial, t_conc


def carried_inplace():
    """one thread: symbolic + numeric of P1, the SAME device buffers rewritten with P2 (same M, K, N), symbolic into the same crpt, numeric: P2's product.

    This pins the sequence end to end with integer values; it is not the test with teeth for a stale carried state. g4s_spgemm_symbolic always replaces
    the state it keeps, and g4s_spgemm_numeric takes a kept state over only while the index arrays still hash to what the symbolic call saw, so no
    single host-side mistake makes this variant fail (a symbolic call that kept a state matching in M, K, N alone still gave P2's product: the hash
    check discarded it). The hash check itself is what test_spgemm_gpu.py::test_spgemm_two_call_form_carries_its_columns pins."""
    Ps = cc.products()[:2]
    for P in Ps:
        prepare(P)
    cap = max(P.nnz for P in Ps)
    rp = torch.empty(Ps[0].n + 1, dtype=torch.int32, device="cuda")
    ci = torch.zeros(cap, dtype=torch.int32, device="cuda")
    va = torch.zeros(cap, dtype=torch.float64, device="cuda")
    crpt = torch.empty(Ps[0].n + 1, dtype=torch.int32, device="cuda")
    src = [(up(P.A[0]), up(P.A[1]), up(P.A[2])) for P in Ps]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    class View:                                                     # what symbolic() / numeric() read of a Dev
        pass

    def work():
        with torch.cuda.stream(stream):
            for r in range(cc.ROUNDS):
                for k, P in enumerate(Ps):
                    rp.copy_(src[k][0]); ci[:P.nnz].copy_(src[k][1]); va[:P.nnz].copy_(src[k][2])
                    d = View()
                    d.P, d.rp, d.ci, d.va = P, rp, ci, va
                    what = f"in place round {r} {P.name}"
                    if symbolic(d, crpt, what):
                        numeric(d, crpt, "plus_times" if (r + k) % 2 == 0 else "min_plus", what)
            stream.synchronize()
    t_serial = timed(work)
    ok("g4s_trim", lib.g4s_trim())
    return t_serial, t_serial                                       # one thread: there is no second way to run it


# ------------------------------------------------------------------------------------------------ d. errors_stay_with_their_thread
A_WORDS = ("a column id is outside", "strictly ascending", "k is negative")


def errors_stay_with_their_thread():
    P = cc.products()[0]
    for Q in cc.products():
        prepare(Q)
    d = Dev(P)
    devs = [d, Dev(cc.products()[1]), Dev(cc.products()[2])]
    bad_ci, bad_mask = (up(a) for a in cc.invalid_inputs())
    ctxs = [ThreadCtx(i) for i in range(3)]
    for t in ctxs[1:]:
        t.traversal = Traversal(cc.products()[t.index % 3])
    hA = host.CSR.from_host(*P.A, P.n, P.n)
    hA.spmm_reserve(8)
    X = up(cc.int_vector(5, P.n, 8))
    Y = torch.zeros(P.n, 8, dtype=torch.float64, device="cuda")
    labels = torch.empty(P.n, dtype=torch.int32, device="cuda")
    cval = torch.empty(P.nnz, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def refused(what, status, word, fn_name):
        called()
        text = lib.g4s_last_error().decode()
        if status != capi.ERR_INVALID:
            differ(f"A: {what}: status {status}, expected G4S_ERR_INVALID")
        if word not in text or fn_name not in text:
            differ(f"A: {what}: g4s_last_error() is not this call's: {text!r}")

    def bad_components():
        refused("bad column id", lib.g4s_connected_components(P.n, dptr(d.rp), dptr(bad_ci), dptr(labels), DEV, None, cur()), A_WORDS[0], "g4s_connected_components")

    def bad_masked():
        refused("unsorted mask", lib.g4s_spgemm_masked(P.n, P.n, P.n, dptr(d.rp), dptr(d.ci), dptr(d.va), dptr(d.rp), dptr(d.ci), dptr(d.va), dptr(d.rp), dptr(bad_mask),
                                                       dptr(cval), DEV, None, cur()), A_WORDS[1], "g4s_spgemm_masked")

    def bad_spmm():
        refused("negative k", lib.g4s_spmm(hA.handle, -1, dptr(X), 8, dptr(Y), 8, 1.0, 0.0, 0, cur()), A_WORDS[2], "g4s_spmm")

    mode = {"concurrent": False}                                   # (run serially, all three share the main thread and its message: nothing to check)

    def valid(i, k):
        def f():
            before = own_differences()                             # (this thread's own: what another thread records at the same time must not hide the check)
            op, p = (i * 7 + k * 3) % len(OPS), (i + k) % 3
            OPS[op][1](ctxs[i], devs[p])
            text = lib.g4s_last_error().decode()
            if mode["concurrent"] and own_differences() == before and any(w in text for w in A_WORDS):
                differ(f"thread {i}: g4s_last_error() shows another thread's refusal after a valid {OPS[op][0]}: {text!r}")
        return f

    a_valid = (lambda: op_components(d, False), lambda: op_masked(d, "plus_times"), lambda: op_onecall_dev(d, "plus_times"), lambda: op_two_call(d, "min_plus"))

    def slots():
        out, k = [], 0
        for r in range(cc.ROUNDS):
            for bad in (bad_components, bad_masked, bad_spmm):
                out.append({0: bad, 1: valid(1, k), 2: valid(2, k)})
                k += 1
            out.append({0: a_valid[r % 4], 1: valid(1, k), 2: valid(2, k)})   # a refusal leaves nothing behind: A's next valid call is exact too
            k += 1
        return out

    t_serial = timed(lambda: lockstep(ctxs, slots(), False))
    _serial_pass[0] = False
    mode["concurrent"] = True
    t_conc = timed(lambda: lockstep(ctxs, slots(), True))
    hA.close()
    return t_serial, t_conc


def main(scenario):
    global lib
    t0 = time.perf_counter()
    assert scenario in SCENARIOS, f"unknown scenario {scenario!r}; one of {SCENARIOS}"
    assert torch.cuda.is_available(), "the concurrency worker needs cuda:0"
    torch.cuda.set_device(0)
    lib = capi.load()
    capi.check(lib.g4s_warm_up())
    run = {"handles_on_streams": handles_on_streams, "threads_synchronous_calls": threads_synchronous_calls, "carried_product": lambda: carried("product"),
           "carried_trim": lambda: carried("trim"), "carried_symbolic": lambda: carried("symbolic"), "carried_inplace": carried_inplace,
           "errors_stay_with_their_thread": errors_stay_with_their_thread}[scenario]
    t_serial, t_conc = run()
    torch.cuda.synchronize()
    print(json.dumps({"scenario": scenario, "calls": calls[0], "n_differences": len(differences), "differences": differences[:20],
                      "serial_s": round(t_serial, 3), "concurrent_s": round(t_conc, 3), "total_s": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
