#!/usr/bin/env python3
"""g4s_sptrsv_* per matrix: the analysis, the solve, and the two comparators that exist today — scipy's spsolve_triangular on the host for the same
triangle, and g4s_spmv of the same triangle on the device, the floor: a solve reads the same bytes, so solve / SpMV is the price of the dependencies.
  lap5      the lower triangle of the configs[0] grid (1000 × 1000, 5-point): 1999 levels of at most 1000 rows
  lap7      the lower triangle of a 128³ seven-point stencil: 382 levels
  rmat_sym  the lower triangle of configs[1] symmetrised, unit diagonal, every value 0.5 / its row's length: wide, shallow, with hubs
  bidiag    a bidiagonal matrix of 10⁵ rows: a level per row, the worst case
One JSON line per matrix: analyse_ms (one cold call included in `analyse_ms_first`), solve_ms and solve_nochains_ms (median, min, max over --reps
windows of --solves solves each, the two variants alternating, after one untimed window), spmv_ms the same way, solve_over_spmv, analysis_in_solves,
launches per solve with and without chains, levels_ok (the levels against their definition, computed with torch at this size), scipy_ms (one timed run, skipped above --scipy-max entries) with the largest relative difference of the
two solutions, and the time of a Gauss–Seidel sweep (g4s_spmv + one solve + two vector operations) against a Jacobi sweep (g4s_spmv + a scale).
Usage: python tools/bench_trsv.py [--matrices lap5,lap7,rmat_sym,bidiag] [--small] [--reps 5] [--solves 20] [--no-scipy]
With --rhs 1,2,4,… it measures the block solve instead (g4s_sptrsv_solve_multi; profiles/trsm.txt), on lap5, lap7 and bidiag unless
--matrices says otherwise: one JSON line per matrix and k with multi_ms (row-major) and multi_colmajor_ms (median, min, max over --reps windows, one
untimed window first, the two layouts and the single solve alternating in every round), k_singles_ms = k × the single solve measured in the same
rounds on the same plan, their ratio, the kernels either way enqueues, and whether every column of both blocks has the single solve's bits. The same
for g4s_ilu0_apply_multi on lap5 ("op": "ilu0_apply"). A window is --solves calls, fewer where one call takes long: about --window-ms of work."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kcore import wall  # noqa: E402


def build(name, host, small):
    """(A: a device CSR holding at least the lower triangle, unit_diagonal)"""
    import torch
    from bench import build_matrix
    if name == "lap5":
        return build_matrix("lap5", host, small), False
    if name == "lap7":
        s = 128 if not small else 40
        return host.laplacian_csr(7, s, s, s), False
    if name == "rmat_sym":
        from bench_components import symmetrise
        R = build_matrix("rmat", host, small)
        rp, ci = symmetrise(R.rowptr, R.colids, R.rows)
        n = R.rows
        del R
        length = (rp[1:] - rp[:-1]).clamp(min=1).double()
        va = torch.repeat_interleave(0.5 / length, (rp[1:] - rp[:-1]).long())
        return host.CSR(rp, ci, va, n, n), True
    if name == "bidiag":
        n = 100_000 if not small else 5_000
        i = torch.arange(n, dtype=torch.int32, device="cuda")
        rp = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), (2 * i + 1)])
        ci = torch.stack([i - 1, i], 1).reshape(-1)[1:].contiguous()
        va = torch.tensor([-1.0, 2.5], dtype=torch.float64, device="cuda").repeat(n)[1:].contiguous()
        return host.CSR(rp, ci, va, n, n), False
    raise SystemExit(f"unknown matrix {name}")


def windows(variants, reps, count):
    """median / min / max ms per call of each variant: `reps` timed windows of count[variant] calls, the variants alternating, after one untimed window"""
    times = {k: [] for k in variants}
    for rep in range(reps + 1):
        for key, fn in variants.items():
            ms, _ = wall(lambda: [fn() for _ in range(count[key])])
            if rep:
                times[key].append(ms / count[key])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def rhs_lines(name, op, n, one, multi, info_launches, ks, args):
    """The lines of one matrix and one operation. one(b, out): the single call; multi(B, out): the block call; b is scaled per column so that every
    column differs; the blocks are allocated per k and released before the next."""
    import torch
    from g4s_amd import host
    b = host.synth_vector(7, n)
    x = torch.empty_like(b)
    est, _ = wall(lambda: one(b, x))
    est, _ = wall(lambda: one(b, x))
    for k in ks:
        scale = 1.0 + torch.arange(k, dtype=torch.float64, device="cuda") / 8.0
        Br = (b[:, None] * scale[None, :]).contiguous()
        Bc = Br.t().contiguous().t()                                         # the same block, column-major with ld = n
        Xr, Xc = torch.empty_like(Br), torch.empty_like(Bc.t()).t()
        assert Bc.stride() == (1, n) or k == 1
        est_k, _ = wall(lambda: multi(Br, Xr))
        count = lambda ms: max(1, min(args.solves, int(args.window_ms / max(ms, 1e-3))))
        t = windows({"single": lambda: one(b, x), "multi": lambda: multi(Br, Xr), "multi_colmajor": lambda: multi(Bc, Xc)}, args.reps,
                    {"single": count(est), "multi": count(est_k), "multi_colmajor": count(est_k)})
        same = True
        for j in sorted({0, k // 2, k - 1}):                                # three columns by bits: the block against the single solve of that column
            one(Br[:, j].contiguous(), x)
            same = same and bool(torch.equal(x.view(torch.int64), Xr[:, j].contiguous().view(torch.int64)))
            same = same and bool(torch.equal(x.view(torch.int64), Xc[:, j].contiguous().view(torch.int64)))
        line = {"bench": "trsm", "op": op, "matrix": name, "n": n, "k": k, "kernels_multi": info_launches, "kernels_k_singles": k * info_launches,
                "columns_equal_single_solves": same}
        for key in ("multi", "multi_colmajor", "single"):
            med, lo, hi = t[key]
            line[key + "_ms"], line[key + "_ms_min"], line[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
        line["k_singles_ms"] = round(k * t["single"][0], 4)
        line["multi_over_k_singles"] = round(t["multi"][0] / (k * t["single"][0]), 4)
        line["colmajor_over_rowmajor"] = round(t["multi_colmajor"][0] / t["multi"][0], 3)
        line["multi_ms_per_column"] = round(t["multi"][0] / k, 4)
        print(json.dumps(line), flush=True)
        del Br, Bc, Xr, Xc


def rhs_main(args):
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    ks = [int(v) for v in args.rhs.split(",")]
    names = (args.matrices or "lap5,lap7,bidiag").split(",")
    for name in names:
        A, unit = build(name, host, args.small)
        plan = host.sptrsv_analyse(A, unit_diagonal=unit)
        rhs_lines(name, "sptrsv_solve", A.rows, lambda b, out: plan.solve(b, out=out), lambda B, out: plan.solve(B, out=out),
                  plan.info["launches_per_solve"], ks, args)
        plan.close()
        if name == "lap5":
            M = host.ilu0(A)
            rhs_lines(name, "ilu0_apply", A.rows, lambda r, out: M.apply(r, out=out), lambda R, out: M.apply(R, out=out), M.info["launches_per_apply"], ks, args)
            M.close()
        del A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=None, help="default: lap5,lap7,rmat_sym,bidiag; with --rhs: lap5,lap7,bidiag")
    ap.add_argument("--rhs", default=None, help="k1,k2,…: measure the block solve of k right-hand sides against k single solves")
    ap.add_argument("--window-ms", type=float, default=200.0, help="--rhs: a timed window is about this much work, at least one call")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-max", type=int, default=20_000_000)
    args = ap.parse_args()
    if args.rhs:
        return rhs_main(args)
    args.matrices = args.matrices or "lap5,lap7,rmat_sym,bidiag"
    import numpy as np
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.matrices.split(","):
        A, unit = build(name, host, args.small)
        n = A.rows
        first, plan = wall(lambda: host.sptrsv_analyse(A, unit_diagonal=unit))
        plan.close()
        analyse = []
        for _ in range(3):
            ms, plan = wall(lambda: host.sptrsv_analyse(A, unit_diagonal=unit))
            analyse.append(ms)
            plan.close()
        plan, level = host.sptrsv_analyse(A, unit_diagonal=unit, return_level=True)
        # the levels checked at this size by their definition, with torch: level[i] = max over the triangle's off-diagonal entries of level[col] + 1, else 0
        row = host.csr_row_indices(A.rowptr, A.nnz).long()
        dep = A.colids.long() < row
        want = torch.zeros(n, dtype=torch.int32, device="cuda").scatter_reduce_(0, row[dep], level[A.colids.long()[dep]] + 1, "amax")
        levels_ok = bool(torch.equal(want, level))
        del row, dep, want, level
        flat = host.sptrsv_analyse(A, unit_diagonal=unit, no_chains=True)
        T = host.csr_select(A, "tril", -1 if unit else 0)                     # the triangle itself, for the floor and for scipy
        b = host.synth_vector(7, n)
        x, xf, y = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
        T.spmv(b, y)
        per = lambda launches: max(1, min(args.solves, 40_000 // max(launches, 1)))   # a window of at most 40 000 launches: the bidiagonal one is 10⁵ a solve
        t = windows({"solve": lambda: plan.solve(b, out=x), "solve_nochains": lambda: flat.solve(b, out=xf), "spmv": lambda: T.spmv(b, y)}, args.reps,
                    {"solve": per(plan.info["launches_per_solve"]), "solve_nochains": per(flat.info["launches_per_solve"]), "spmv": args.solves})
        assert torch.equal(x, xf)
        line = {"bench": "trsv", "matrix": name, "n": n, "unit_diagonal": unit, **{k: plan.info[k] for k in ("nnz_triangle", "levels", "widest_level", "chains")},
                "launches_per_solve": plan.info["launches_per_solve"], "launches_per_solve_nochains": flat.info["launches_per_solve"],
                "analyse_ms_first": round(first, 3), "analyse_ms": round(statistics.median(analyse), 3), "analyse_launches": plan.info["launches"],
                "analyse_host_waits": plan.info["host_waits"], "levels_ok": levels_ok}
        for k, (med, lo, hi) in t.items():
            line[k + "_ms"], line[k + "_ms_min"], line[k + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
        line["solve_over_spmv"] = round(t["solve"][0] / t["spmv"][0], 2)
        line["analysis_in_solves"] = round(statistics.median(analyse) / t["solve"][0], 1)
        # a Gauss–Seidel sweep against a Jacobi sweep on the whole matrix (unit: D = I)
        xs = torch.zeros_like(b)
        if unit:
            dinv = torch.ones_like(b)
        else:
            row = host.csr_row_indices(A.rowptr, A.nnz).long()
            dinv = 1.0 / torch.zeros_like(b).scatter_add_(0, row, torch.where(A.colids.long() == row, A.values, torch.zeros_like(A.values)))
            del row
        r = torch.empty_like(b)

        def jacobi():
            r.copy_(b)
            A.spmv(xs, r, alpha=-1.0, beta=1.0)
            xs.addcmul_(r, dinv)

        A.spmv(b, y)
        sweeps = windows({"gauss_seidel": lambda: host.gauss_seidel(A, b, xs, 1, plans=(plan, None)), "jacobi": jacobi}, args.reps,
                         {"gauss_seidel": per(plan.info["launches_per_solve"]), "jacobi": args.solves})
        line["gauss_seidel_sweep_ms"], line["jacobi_sweep_ms"] = round(sweeps["gauss_seidel"][0], 4), round(sweeps["jacobi"][0], 4)
        if not args.no_scipy and plan.info["nnz_triangle"] <= args.scipy_max:
            import time
            import scipy.sparse as sp
            from scipy.sparse.linalg import spsolve_triangular
            rp, ci, va = T.to_host()
            M = sp.csr_matrix((va, ci, rp), shape=(n, n))
            if unit:
                M = (M + sp.identity(n, format="csr")).tocsr()
            bh = b.cpu().numpy()
            t0 = time.perf_counter()
            xh = spsolve_triangular(M, bh, lower=True)
            line["scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            got = x.cpu().numpy()
            line["max_rel_diff_to_scipy"] = float(np.max(np.abs(got - xh) / np.maximum(np.abs(xh), 1e-300)))
        print(json.dumps(line), flush=True)
        plan.close()
        flat.close()
        del A, T


if __name__ == "__main__":
    main()
