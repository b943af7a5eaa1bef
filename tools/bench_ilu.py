#!/usr/bin/env python3
"""g4s_ilu0_* per matrix: the analysis (which ends with the first factorisation), a refactorisation, the apply, and the two comparators that exist —
g4s_sptrsv_solve on the same strictly lower triangle (the factorisation runs on that plan's schedule, so factor / solve is the price of the pivot
loops over the solve's dependent launches), and the row-wise ILU(0) loop in plain Python on the host (scipy has none), whose floats are the
device's bit for bit.
  lap5      the configs[0] grid (1000 × 1000, 5-point): 1999 levels of at most 1000 rows
  lap7      a 128³ seven-point stencil: 382 levels
  rmat_sym  configs[1] symmetrised, a unit diagonal added, every other value −0.5 / its row's length: wide, shallow, with hubs
  bidiag    a bidiagonal matrix of 10⁵ rows: a level per row, the worst case
One JSON line per matrix: analyse_ms (one cold call in `analyse_ms_first`), factor_ms and factor_nochains_ms, apply_ms and solve_ms (median, min, max
over --reps windows of --calls calls each, the variants alternating, after one untimed window; a window is cut to at most 40 000 launches and to
about --window-ms), factor_over_solve, analysis_in_factors, the launch counts, factors_equal (with and without chains), and host_loop_ms (one timed
run, skipped above --host-max entries) with host_equal: the device's factors against the host loop's, bit for bit.
Usage: python tools/bench_ilu.py [--matrices lap5,lap7,rmat_sym,bidiag] [--small] [--reps 5] [--calls 20] [--window-ms 2000] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kcore import wall  # noqa: E402
from bench_trsv import windows  # noqa: E402


def build(name, host, small):
    """A: a device CSR with canonical rows that stores its diagonal"""
    import torch
    from bench import build_matrix
    if name == "lap5":
        return build_matrix("lap5", host, small)
    if name == "lap7":
        s = 128 if not small else 40
        return host.laplacian_csr(7, s, s, s)
    if name == "rmat_sym":
        from bench_components import symmetrise
        R = build_matrix("rmat", host, small)
        n = R.rows
        rp, ci = symmetrise(R.rowptr, R.colids, n)
        del R
        S = host.CSR(rp, ci, torch.ones(ci.numel(), dtype=torch.float64, device="cuda"), n, n)
        eye = torch.arange(n + 1, dtype=torch.int32, device="cuda")
        U = host.csr_ewise(S, host.CSR(eye, eye[:n].contiguous(), torch.ones(n, dtype=torch.float64, device="cuda"), n, n), "union", "first")
        del S
        row = host.csr_row_indices(U.rowptr, U.nnz).long()
        length = (U.rowptr[1:] - U.rowptr[:-1]).double()
        va = torch.where(U.colids.long() == row, torch.ones_like(U.values), (-0.5 / length)[row])
        return host.CSR(U.rowptr, U.colids, va, n, n)
    if name == "bidiag":
        n = 100_000 if not small else 5_000
        i = torch.arange(n, dtype=torch.int32, device="cuda")
        rp = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), (2 * i + 1)])
        ci = torch.stack([i - 1, i], 1).reshape(-1)[1:].contiguous()
        va = torch.tensor([-1.0, 2.5], dtype=torch.float64, device="cuda").repeat(n)[1:].contiguous()
        return host.CSR(rp, ci, va, n, n)
    raise SystemExit(f"unknown matrix {name}")


def host_ilu0(rp, ci, va):
    """the row-wise loop of include/g4s.h on Python floats (IEEE doubles, no FMA): the factor array"""
    f = list(va)
    n = len(rp) - 1
    dpos = [0] * n
    for i in range(n):
        rb, re = rp[i], rp[i + 1]
        pos = {ci[q]: q for q in range(rb, re)}
        dpos[i] = pos[i]
        for p in range(rb, re):
            k = ci[p]
            if k >= i:
                break
            wp = f[p] / f[dpos[k]]
            f[p] = wp
            for q in range(dpos[k] + 1, rp[k + 1]):
                t = pos.get(ci[q])
                if t is not None:
                    f[t] = f[t] - wp * f[q]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="lap5,lap7,rmat_sym,bidiag")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=2000.0, help="a timed window is cut to about this long, judged by the first analysis")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max", type=int, default=20_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.matrices.split(","):
        A = build(name, host, args.small)
        n = A.rows
        first, M = wall(lambda: host.ilu0(A))
        M.close()
        analyse = []
        for _ in range(3 if first < args.window_ms else 0):                 # a slow factorisation (hub rows) is timed once
            ms, M = wall(lambda: host.ilu0(A))
            analyse.append(ms)
            M.close()
        analyse = analyse or [first]
        M, flat = host.ilu0(A), host.ilu0(A, no_chains=True)
        plan = host.sptrsv_analyse(A, unit_diagonal=True)                   # the solve on the same strictly lower triangle
        r = host.synth_vector(7, n)
        z, x = torch.empty_like(r), torch.empty_like(r)
        # a window of at most 40 000 launches and, by the time of the first analysis, of about --window-ms
        per = lambda launches: max(1, min(args.calls, 40_000 // max(launches, 1), int(args.window_ms / max(first, 1e-3))))
        t = windows({"factor": lambda: M.factor(), "factor_nochains": lambda: flat.factor(), "apply": lambda: M.apply(r, out=z), "solve": lambda: plan.solve(r, out=x)},
                    args.reps, {"factor": per(M.info["launches_per_factor"]), "factor_nochains": per(flat.info["launches_per_factor"]),
                                "apply": per(M.info["launches_per_apply"]), "solve": per(plan.info["launches_per_solve"])})
        f = M.factors()
        line = {"bench": "ilu0", "matrix": name, **{k: M.info[k] for k in ("n", "nnz", "levels", "widest_level", "chains", "launches_per_factor", "launches_per_apply",
                                                                        "bad_pivot")},
                "launches_per_factor_nochains": flat.info["launches_per_factor"], "analyse_ms_first": round(first, 3), "analyse_ms": round(statistics.median(analyse), 3),
                "analyse_launches": M.info["launches"], "analyse_host_waits": M.info["host_waits"],
                "factors_equal": bool(torch.equal(f.view(torch.int64), flat.factors().view(torch.int64)))}
        for k, (med, lo, hi) in t.items():
            line[k + "_ms"], line[k + "_ms_min"], line[k + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
        line["factor_over_solve"] = round(t["factor"][0] / t["solve"][0], 2)
        line["analysis_in_factors"] = round(statistics.median(analyse) / t["factor"][0], 1)
        if not args.no_host and A.nnz <= args.host_max:
            rp, ci, va = (a.tolist() for a in A.to_host())
            t0 = time.perf_counter()
            fh = host_ilu0(rp, ci, va)
            line["host_loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            line["host_equal"] = bool(np.array_equal(np.array(fh).view(np.int64), f.cpu().numpy().view(np.int64)))
        print(json.dumps(line), flush=True)
        M.close()
        flat.close()
        plan.close()
        del A


if __name__ == "__main__":
    main()
