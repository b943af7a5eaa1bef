"""The device-resident CG loop of csrc/cg.hip (g4s_conj_grad, g4s_conj_grad_node, the g4s_cg_* step API, g4s_conj_grad_dist) against a longdouble
restatement of the same loop (tests/cg_ref.py), iteration by iteration: every cap, the exact stopping iteration, batch independence bit for bit,
no memory of the previous solve, the degenerate starts, a caller's stream, the step API, reproducibility, the one-rank distributed loop.

The bound rule (no tolerance fixed in advance): for each compared iterate or residual, gap = max|cg_ref float64 − cg_ref longdouble| / max|longdouble|
(neither side is the code under test; asserted <= 1e-10, see tests/test_cg_ref_cpu.py), and the device must satisfy
max|device − longdouble| / max|longdouble| <= 16·max(gap, 2⁻⁵⁰). The device adds in a third order (256-way two-level dot products, a mat-vec order
per SpMV path) and CG feeds each rounding back through alpha and beta: hence the factor 16.

Two places where the cases cannot be taken literally. (1) neq = 1: CG is exact after one iteration, so the residual after it and everything a further
iteration does are round-off of the run itself (the longdouble run stops at 2 iterations on a residual of exactly 0, the float64 run at 11). There the
iterate is compared for caps 0 and 1, the residual must be <= 16·2⁻⁵⁰·|F|, and for larger caps only 1 <= cycles <= cap is required.
(2) The diagonal SpMV path (3) needs 1024 rows (dia_try_build), so a default handle at neq 257 is on path 0; the trajectory test asserts that and still
runs it, and path 3 gets neq 1025 as its small size in the trajectory, stopping and step-API tests.

Largest observed err / max(gap, 2⁻⁵⁰) on an MI355X (bound: 16), all compared iterates and residuals:
  element operator 1.22, node operator 0.64, CSR path 0 (row-streaming) 3.62, path 1 (blocked) 0.47, path 3 (diagonal) 0.58, path 4 (block-row) 0.55,
  one-rank distributed loop 1.33. The largest, 3.62, is the residual after 12 iterations at neq 257 (err 3.2e-15 against a gap of 6.7e-16).
The module prints every compared figure and, at its end, these maxima (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cg_cases, cg_ref

pytestmark = pytest.mark.gpu

RATIOS = {}                                                       # operator → largest err / max(gap, 2⁻⁵⁰) seen in this run (printed at the end of the module)


# ------------------------------------------------------------------------------------------------ device side
class Dev:
    """One problem on the device with one operator: kind "elem" | "node" | "csr" (flags: the G4S_SPMV_* path flags of the handle)."""

    def __init__(self, p, kind, flags=0):
        from g4s_amd import capi, host
        self.p, self.kind, self.lib, self.capi = p, kind, capi.load(), capi
        self.h, self.A = C.c_void_p(), None
        if kind == "elem":
            self.Kd = torch.from_numpy(p["K"]).cuda()
            capi.check(self.lib.g4s_elem_op_create(C.byref(self.h), len(p["ien"]), 8, 3, np.ascontiguousarray(p["ien"]).ctypes.data,
                                                   np.ascontiguousarray(p["idmap"]).ctypes.data, p["nno"], p["n"], self.Kd.data_ptr()))
        elif kind == "node":
            from tests.test_nodeop_gpu import _create
            self.h = _create(self.lib, capi, p["nno"], p["n"], p["nm"], p["max_eqn"], p["idmap"], p["ks"])
        else:
            rp, ci, va = p["csr"]
            self.A = host.CSR.from_host(rp, ci, va, p["n"], p["n"], spmv_flags=flags)
            self.path = self.A.info()["spmv_path"]
        self.label = kind if kind != "csr" else f"csr path {self.path}"
        self.BI, self.F, self.bc = torch.from_numpy(p["BI"]).cuda(), torch.from_numpy(p["F"]).cuda(), torch.from_numpy(p["bc"]).cuda()
        torch.cuda.synchronize()

    def close(self):
        if self.kind == "elem":
            self.lib.g4s_elem_op_destroy(self.h)
        elif self.kind == "node":
            self.lib.g4s_node_op_destroy(self.h)
        else:
            self.A.close()

    def nan_d0(self):
        """A NaN-filled d0, complete on the device when this returns."""
        d0 = torch.full((self.p["n"],), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return d0

    def solve(self, acc, steps, F=None, bc="list", stream=None, d0=None):
        """(d0, cycles, residual) of the one-call solve; d0 is NaN on entry. bc: "list" (the problem's), "null" (n_zero = 0, NULL), "empty" (n_zero = 0 with a
        pointer), or a device tensor. With a d0 of the caller (nan_d0) nothing here touches the device before the library call: work the caller has
        enqueued is still pending when the solve is."""
        n = self.p["n"]
        F = self.F if F is None else F
        if isinstance(bc, torch.Tensor):
            zp, nz = bc.data_ptr(), bc.numel()
        elif bc == "null":
            zp, nz = None, 0
        elif bc == "empty":
            zp, nz = self.BI.data_ptr(), 0                          # a pointer that is never read
        else:
            assert bc == "list"
            zp, nz = (self.bc.data_ptr(), self.bc.numel()) if self.bc.numel() else (None, 0)
        if d0 is None:
            d0 = self.nan_d0()
        cyc, res = C.c_int32(steps), C.c_double(float("nan"))
        if self.kind == "node":
            st = self.lib.g4s_conj_grad_node(self.h, n, self.BI.data_ptr(), zp, nz, F.data_ptr(), d0.data_ptr(), float(acc), C.byref(cyc), C.byref(res), stream)
        else:
            st = self.lib.g4s_conj_grad(self.h if self.kind == "elem" else None, self.A.handle if self.kind == "csr" else None, n, self.BI.data_ptr(), zp, nz,
                                        F.data_ptr(), d0.data_ptr(), float(acc), C.byref(cyc), C.byref(res), stream)
        self.capi.check(st)
        torch.cuda.synchronize()
        return d0.cpu().numpy(), cyc.value, res.value

    def solve_stepwise(self, acc, steps):
        """The same solve through the step API with g4s_spmv as the product: one rank, no all-reduce (g4s_amd/dist.py:dist_conj_grad without its collectives)."""
        lib, capi, n = self.lib, self.capi, self.p["n"]
        ws = C.c_void_p()
        capi.check(lib.g4s_cg_ws_create(C.byref(ws), n))
        try:
            d0 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            zp, nz = (self.bc.data_ptr(), self.bc.numel()) if self.bc.numel() else (None, 0)
            capi.check(lib.g4s_cg_begin(ws, self.F.data_ptr(), self.BI.data_ptr(), d0.data_ptr(), zp, nz, None))
            p_ptr, Ap_ptr = C.c_void_p(), C.c_void_p()
            count, done, residual = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
            for _ in range(steps + 2):
                capi.check(lib.g4s_cg_direction(ws, int(steps), float(acc), None))
                capi.check(lib.g4s_cg_state(ws, C.byref(count), C.byref(done), C.byref(residual), None))
                if done.value:
                    break
                capi.check(lib.g4s_cg_buffers(ws, C.byref(p_ptr), C.byref(Ap_ptr), None))
                capi.check(lib.g4s_spmv(self.A.handle, p_ptr, Ap_ptr, 1.0, 0.0, None))
                capi.check(lib.g4s_cg_reduce_pAp(ws, None))
                capi.check(lib.g4s_cg_update(ws, self.BI.data_ptr(), d0.data_ptr(), None))
            assert done.value, "the step API never raised its done flag"
            capi.check(lib.g4s_cg_end(ws, d0.data_ptr(), zp, nz, None))
            torch.cuda.synchronize()
            return d0.cpu().numpy(), count.value, residual.value
        finally:
            lib.g4s_cg_ws_destroy(ws)

    def inputs_unchanged(self):
        return np.array_equal(self.F.cpu().numpy(), self.p["F"]) and np.array_equal(self.BI.cpu().numpy(), self.p["BI"]) and np.array_equal(self.bc.cpu().numpy(), self.p["bc"])


@pytest.fixture(scope="module")
def devs(oracle):
    """Device operators, created on first use and shared by the tests of this module. Keys: "elem24", "elem1215", "node", ("band", n, which) with
    which = "stream" (path 0) | "blocked" (path 1) | "default" (path 3 from 1024 rows on) and ("fe", "default"): the assembled element matrix (path 4)."""
    from g4s_amd import capi
    made = {}

    def get(key):
        if key not in made:
            if key == "elem24":
                made[key] = Dev(cg_cases.elem_problem(1, 1, 1, 0, oracle), "elem")
            elif key == "elem1215":
                made[key] = Dev(cg_cases.elem_problem(8, 8, 4, 1, oracle), "elem")
            elif key == "node":
                made[key] = Dev(cg_cases.node_problem(oracle), "node")
            elif key[0] == "fe":
                made[key] = Dev(cg_cases.elem_problem(8, 8, 4, 1, oracle), "csr")
                assert made[key].path == 4, made[key].A.info()
            else:
                _, n, which = key
                d = Dev(cg_cases.band_problem(n), "csr", {"stream": capi.SPMV_STREAM, "blocked": capi.SPMV_BLOCKED, "default": 0}[which])
                want = {"stream": 0, "blocked": 1, "default": 3 if n >= 1024 else 0}[which]   # the diagonal form needs 1024 rows (dia_try_build)
                assert d.path == want, (key, d.A.info())
                made[key] = d
        return made[key]

    yield get
    for d in made.values():
        d.close()
    print("\nlargest err / max(gap, 2^-50) per operator (bound 16):", {k: round(v, 3) for k, v in sorted(RATIOS.items())})


@pytest.fixture(autouse=True)
def _no_batch_override(monkeypatch):
    monkeypatch.delenv("G4S_CG_FIRST_BATCH", raising=False)


def _check(label, what, got, ref_ld, gap, failures):
    """The bound rule for one compared quantity; records the observed ratio, prints the figures, appends a message on a miss."""
    assert gap <= cg_ref.GAP_MAX, (what, gap)                      # precondition (also asserted without a GPU in tests/test_cg_ref_cpu.py)
    err = cg_ref.rel_gap(got, ref_ld) if np.all(np.isfinite(got)) else float("inf")
    ratio = err / max(gap, cg_ref.GAP_FLOOR)
    RATIOS[label] = max(RATIOS.get(label, 0.0), ratio)
    print(f"{label:11s} {what:40s} err {err:.3e} gap {gap:.3e} ratio {ratio:.2f}")
    if not err <= cg_ref.bound(gap):
        failures.append(f"{what}: err {err:.3e} > 16·max(gap {gap:.3e}, 2^-50)")


def _check_iterate(dev, R, k, d0, res, tag, failures):
    """d0 and residual of a device solve that did k iterations against the longdouble reference's k-th iterate."""
    p = dev.p
    if not np.all(d0[p["bc"]] == 0.0):
        failures.append(f"{tag}: d0 is not zero on the boundary list")
    _check(dev.label, f"{p['name']} {tag} d0", d0, R.iterate(k), R.gap_d0(k), failures)
    if cg_cases.comparable_residual(p, k):
        _check(dev.label, f"{p['name']} {tag} residual", res, R.residual(k), R.gap_res(k), failures)
    elif not res <= cg_ref.bound(0.0) * float(np.linalg.norm(p["F"])):
        failures.append(f"{tag}: residual {res:.3e} after the last Krylov dimension is not round-off of |F|")


TRAJECTORY = ["elem24", "elem1215", "node"] + [("band", n, "stream") for n in cg_cases.CSR_SIZES] + \
             [("band", n, w) for w in ("blocked", "default") for n in (257, 65537)] + [("band", 1025, "default")]


# ------------------------------------------------------------------------------------------------ 1. trajectory at every cap
@pytest.mark.parametrize("key", TRAJECTORY, ids=lambda k: k if isinstance(k, str) else f"band{k[1]}-{k[2]}")
def test_trajectory_at_every_cap(devs, key):
    """acc = 0 and *cycles = k: exactly max(k, 1) iterations, and the iterate and residual of exactly that iteration — a no-op that still writes, a cap
    inside a batch, a wrong `steps - enqueued + 1` all show here."""
    dev = devs(key)
    p, R, failures = dev.p, cg_cases.reference(dev.p), []
    for k in cg_cases.CAPS:
        d0, cyc, res = dev.solve(0.0, k)
        want = max(k, 1)
        if not cg_cases.comparable(p, k):                          # neq = 1 past its one Krylov dimension (module docstring)
            if not 1 <= cyc <= want:
                failures.append(f"cap {k}: cycles {cyc} outside [1, {want}]")
            continue
        if cyc != want:
            failures.append(f"cap {k}: cycles {cyc}, expected {want}")
            continue
        _check_iterate(dev, R, want, d0, res, f"cap {k}", failures)
    assert dev.inputs_unchanged(), "F, BI or the boundary list changed"
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 2. exact stopping iteration
STOPPING = ["elem1215", "node"] + [("band", n, w) for n in (257, 65537) for w in ("stream", "blocked")] + [("band", n, "default") for n in (1025, 65537)]


@pytest.mark.parametrize("key", STOPPING, ids=lambda k: k if isinstance(k, str) else f"band{k[1]}-{k[2]}")
def test_exact_stopping_iteration(devs, key):
    """acc halfway (geometrically) between the residuals after k−1 and k iterations, cap 250: the device's own loop test must stop at k, not k ± 1."""
    dev = devs(key)
    p, R, failures = dev.p, cg_cases.reference(dev.p), []
    for k in cg_cases.STOP_AT:
        hi, lo = R.residual(k - 1), R.residual(k)
        assert hi > 1.5 * lo                                        # precondition: round-off cannot move either residual across acc
        acc = float(np.sqrt(hi * lo))
        d0, cyc, res = dev.solve(acc, 250)
        if cyc != k:
            failures.append(f"acc between residuals {k - 1} and {k}: stopped after {cyc}")
            continue
        if not res <= acc:
            failures.append(f"stop at {k}: residual {res} > acc {acc}")
        _check_iterate(dev, R, k, d0, res, f"stop at {k}", failures)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 3. batch independence
def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("key", ["elem1215", ("band", 65537, "stream")], ids=["elem1215", "band65537-stream"])
def test_first_batch_size_changes_no_bit(devs, monkeypatch, key):
    dev = devs(key)
    acc = 1e-8 * float(np.linalg.norm(dev.p["F"]))
    runs = {}
    for batch in ("1", "2", "5", "32", None):
        if batch is None:
            monkeypatch.delenv("G4S_CG_FIRST_BATCH", raising=False)
        else:
            monkeypatch.setenv("G4S_CG_FIRST_BATCH", batch)
        runs[batch] = (dev.solve(acc, 250), dev.solve(0.0, 7))
    conv, capped = runs["1"]
    assert 7 < conv[1] < 250 and conv[2] <= acc and capped[1] == 7
    for batch, (a, b) in runs.items():
        assert _same(a, conv), f"converged solve differs between G4S_CG_FIRST_BATCH=1 and {batch}: cycles {a[1]} vs {conv[1]}, residual {a[2]!r} vs {conv[2]!r}"
        assert _same(b, capped), f"solve capped at 7 differs between G4S_CG_FIRST_BATCH=1 and {batch}: cycles {b[1]}, residual {b[2]!r} vs {capped[2]!r}"


# ------------------------------------------------------------------------------------------------ 4. no memory of the previous solve
def test_previous_solve_leaves_no_trace(devs, monkeypatch):
    """P (neq 65 537, 12 iterations), Q (neq 257, cap 2), P again: the thread's remembered iteration count sizes Q's first batch from P and P's from Q, and
    Q's smaller work arena is asked of the scratch pool right after P gave back a larger one, unzeroed. Whatever the pool hands out, the results must not move."""
    P, Q = devs(("band", 65537, "stream")), devs(("band", 257, "stream"))
    p1 = P.solve(0.0, 12)
    q1 = Q.solve(0.0, 2)
    p2 = P.solve(0.0, 12)
    assert p1[1] == 12 and q1[1] == 2
    assert _same(p1, p2), "P after Q differs from P before Q"
    monkeypatch.setenv("G4S_CG_FIRST_BATCH", "1")
    assert _same(q1, Q.solve(0.0, 2)), "Q after P differs from Q with a first batch of 1"
    assert _same(p1, P.solve(0.0, 12))


# ------------------------------------------------------------------------------------------------ 5. degenerate starts
DEGENERATE = ["elem1215", "node", ("band", 257, "stream"), ("band", 65537, "stream")]


@pytest.mark.parametrize("key", DEGENERATE, ids=lambda k: k if isinstance(k, str) else f"band{k[1]}-{k[2]}")
def test_degenerate_starts(devs, key):
    dev = devs(key)
    p, R, failures, n = dev.p, cg_cases.reference(dev.p), [], dev.p["n"]
    # F = 0: the count == 0 clause runs one iteration on a zero direction (pAp == 0 → alpha = 1e-3)
    d0, cyc, res = dev.solve(1e-8, 250, F=torch.zeros(n, dtype=torch.float64, device="cuda"))
    assert cyc == 1 and res == 0.0 and not d0.any(), (cyc, res)
    # acc >= |F| at the start: one iteration still runs
    d0, cyc, res = dev.solve(2.0 * float(np.linalg.norm(p["F"])), 250)
    assert cyc == 1, cyc
    _check_iterate(dev, R, 1, d0, res, "acc = 2|F|", failures)
    # every equation on the boundary list, F != 0, cap 3: Ap is all zero, alpha = 1e-3 three times, r never changes
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    d0, cyc, res = dev.solve(0.0, 3, bc=every)
    normF = float(np.sqrt(np.sum(np.asarray(p["F"], np.longdouble) ** 2)))
    assert cyc == 3 and not d0.any() and np.all(np.isfinite(d0)), cyc
    assert abs(res - normF) <= 4 * np.spacing(normF), (res, normF)
    # n_zero = 0 with a NULL list: the bits of an empty non-NULL list; against the reference not for the node form, whose matrix has the boundary columns
    # dropped at construction (the list only strips rows), so that without a list it is another operator than the assembled K
    a, b = dev.solve(0.0, 4, bc="null"), dev.solve(0.0, 4, bc="empty")
    assert a[1] == 4 and _same(a, b), "a NULL list and an empty list give different bits"
    if dev.kind != "node":
        Rn = cg_cases.Reference(p, steps=4, bc=np.zeros(0, np.int32))
        _check(dev.label, f"{p['name']} no boundary list d0", a[0], Rn.iterate(4), Rn.gap_d0(4), failures)
        _check(dev.label, f"{p['name']} no boundary list residual", a[2], Rn.residual(4), Rn.gap_res(4), failures)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 6. a stream of the caller
def test_solve_on_a_callers_stream(devs):
    """F is filled on the caller's (non-blocking) stream behind a long queue of fills, and the solve is called at once, with nothing synchronising in between:
    the fill is still pending when the solve is enqueued, and a kernel of the solve that ran on another stream would read the NaNs F holds until then."""
    dev = devs(("band", 65537, "stream"))
    want = dev.solve(0.0, 12)
    s = torch.cuda.Stream()
    Fs = torch.full((dev.p["n"],), float("nan"), dtype=torch.float64, device="cuda")
    ballast = torch.empty(1 << 27, dtype=torch.float64, device="cuda")
    d0 = dev.nan_d0()                                              # (synchronises: the last device-wide wait before the library call)
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        for i in range(16):
            ballast.fill_(float(i))
        Fs.copy_(dev.F, non_blocking=True)
        done.record(s)
    pending = not done.query()
    got = dev.solve(0.0, 12, F=Fs, stream=C.c_void_p(s.cuda_stream), d0=d0)
    assert pending, "the fill of F had already run when the solve was called: the queue in front of it is too short to test anything"
    assert want[1] == 12 and _same(got, want), (got[1], got[2], want[2])


# ------------------------------------------------------------------------------------------------ 7. step API == one call
@pytest.mark.parametrize("n,which", [(257, "stream"), (65537, "stream"), (1025, "default"), (65537, "default")])
def test_step_api_equals_one_call(devs, n, which):
    """Paths 0 and 3 (the diagonal form exists from 1024 rows on: 1025 is its small size)."""
    dev = devs(("band", n, which))
    acc = 1e-6 * float(np.linalg.norm(dev.p["F"]))
    for a, steps in ((acc, 250), (0.0, 3)):
        one, step = dev.solve(a, steps), dev.solve_stepwise(a, steps)
        assert one[1] == step[1] and (steps == 250 or one[1] == 3), (one[1], step[1])
        assert _same(one, step), f"acc {a} steps {steps}: count {one[1]} / {step[1]}, residual {one[2]!r} / {step[2]!r}, d0 equal: {np.array_equal(one[0], step[0])}"


# ------------------------------------------------------------------------------------------------ 8. reproducibility
REPRODUCIBLE = ["elem1215", "node", ("band", 65537, "stream"), ("band", 65537, "default"), ("fe", "default")]


@pytest.mark.parametrize("key", REPRODUCIBLE, ids=lambda k: k if isinstance(k, str) else "-".join(str(x) for x in k))
def test_two_solves_give_the_same_bits(devs, key):
    """Not the blocked path: its LDS atomic sums move in the last bits (bound rule and exact count only, tests 1 and 2)."""
    dev = devs(key)
    acc = 1e-8 * float(np.linalg.norm(dev.p["F"]))
    a, b = dev.solve(acc, 250), dev.solve(acc, 250)
    assert a[2] <= acc and _same(a, b)
    a, b = dev.solve(0.0, 12), dev.solve(0.0, 12)
    assert _same(a, b)
    failures = []
    _check_iterate(dev, cg_cases.reference(dev.p), 12, a[0], a[2], "cap 12", failures)   # (path 4 is compared with the reference here only)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ 9. distributed loop, one rank
def test_dist_loop_one_rank_caps_and_batches(oracle, monkeypatch):
    """g4s_conj_grad_dist over the library's RCCL communicator in loopback (set up as test_conj_grad_dist_c_entry_point_over_rccl_loopback), acc = 0."""
    from g4s_amd import capi, dist as gdist
    p = cg_cases.dist_problem(oracle)
    R, n, failures = cg_cases.reference(p), p["n"], []
    rp, ci, va = p["csr"]
    D = gdist.DistSpMV([0, n], 0, 1, torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda(), n, loopback=True)
    try:
        assert D.info()["nnz_rem"] > 0
        BI, Fd, bcd = torch.from_numpy(p["BI"]).cuda(), torch.from_numpy(p["F"]).cuda(), torch.from_numpy(p["bc"]).cuda()
        out = {}
        for cap in (1, 5):
            for batch in ("1", "32"):
                monkeypatch.setenv("G4S_CG_FIRST_BATCH", batch)
                d0 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                cycles, res = C.c_int32(0), C.c_double(float("nan"))
                torch.cuda.synchronize()
                capi.check(capi.load().g4s_conj_grad_dist(D.h, D.comm, n, BI.data_ptr(), bcd.data_ptr(), len(p["bc"]), Fd.data_ptr(), d0.data_ptr(), 0.0, cap,
                                                          C.byref(cycles), C.byref(res), None))
                torch.cuda.synchronize()
                out[cap, batch] = (d0.cpu().numpy(), cycles.value, res.value)
                assert cycles.value == cap, (cap, batch, cycles.value)
            assert _same(out[cap, "1"], out[cap, "32"]), f"cap {cap}: first batches 1 and 32 differ"
            d0, _, res = out[cap, "1"]
            assert np.all(d0[p["bc"]] == 0.0)
            _check("dist", f"{p['name']} cap {cap} d0", d0, R.iterate(cap), R.gap_d0(cap), failures)
            _check("dist", f"{p['name']} cap {cap} residual", res, R.residual(cap), R.gap_res(cap), failures)
        print("dist ratio:", RATIOS.get("dist"))
        assert not failures, failures
    finally:
        D.close()
