#!/usr/bin/env python3
"""g4s_pagerank against the host loop of INTEGRATION.md, on rmat = configs[1] (10M R-MAT, 98.7M edges, weights 1, blocked path), lap5 = the pattern of
configs[0] (1000 × 1000 5-point grid, weights 1) and rmat20s = R-MAT-20 at edge factor 16, symmetrised (weights 1, G4S_PAGERANK_SYMMETRIC). Per graph,
in one process and alternating the variants round by round (--reps rounds after one untimed round):
  loop     (a) the comparator: spmv_transpose + torch vector operations + one .item() per iteration — the only thing a user can write without the call
  call     g4s_pagerank (after pagerank_reserve)
  product  (b) one transposed product alone, the floor per iteration (the mean of `iterations` back-to-back products)
One JSON line per variant: ms (median), ms_min, ms_max, ms_per_iteration, iterations, products, host_waits, residual; `l1_to_loop` is the L1 distance of
the call's ranks from the loop's. The byte model per iteration above the product: 8·n·5 (y, r and 1 / s read, r and x written), + 8·n with a
teleport vector. The epilogue's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_pagerank.py --only call` run.
Usage: python tools/bench_pagerank.py [--graphs rmat,lap5,rmat20s] [--small] [--reps 3] [--damping 0.85] [--tol 1e-10] [--cap 100] [--only call]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def pagerank_loop(A, damping, tol, cap, symmetric):
    """The loop of INTEGRATION.md: networkx's iteration on device tensors, one host read of the residual per iteration."""
    import torch
    n = A.rows
    s = A.spmv(torch.ones(n, dtype=torch.float64, device="cuda"))   # out-strengths
    dangling = s == 0
    inv_s = torch.where(dangling, torch.zeros_like(s), 1.0 / s)
    p = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    r, k, res = p.clone(), 0, 0.0
    product = A.spmv if symmetric else A.spmv_transpose
    while k < cap:
        y = product(r * inv_s)
        m = r[dangling].sum()
        rn = damping * (y + m * p) + (1.0 - damping) * p
        res = (rn - r).abs().sum().item()
        r, k = rn, k + 1
        if res < tol:
            break
    return r, {"iterations": k, "products": k, "host_waits": k, "residual": res}


def symmetrised_rmat(host, scale, edge_factor):
    import torch
    n = 1 << scale
    G = host.rmat_csr(n, scale, edge_factor << scale, 20240521)
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (G.rowptr[1:] - G.rowptr[:-1]).long())
    cols = G.colids.long()
    keys = torch.unique(torch.cat([rows * n + cols, cols * n + rows]))
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return host.CSR(rowptr.to(torch.int32), (keys % n).to(torch.int32), torch.ones(keys.numel(), dtype=torch.float64, device="cuda"), n, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="rmat,lap5,rmat20s")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--damping", type=float, default=0.85)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--only", default="", help="run one variant only (for a profiler)")
    args = ap.parse_args()
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        symmetric = name == "rmat20s"
        if symmetric:
            A = symmetrised_rmat(host, 20 if not args.small else 14, 16)
        else:
            A = build_matrix(name, host, args.small)
            if name == "rmat":
                A._spmv_flags = capi.SPMV_BLOCKED
            A.values.fill_(1.0)
        torch.cuda.synchronize()
        A.pagerank_reserve(symmetric=symmetric)
        path = A.info()["spmv_path"] if symmetric else A.transpose_info()["spmv_path"]
        x = torch.rand(A.rows, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        iters = {"n": args.cap}

        def products():
            f = A.spmv if symmetric else A.spmv_transpose
            for _ in range(iters["n"]):
                f(x, y)
            return None, {"iterations": iters["n"], "products": iters["n"], "host_waits": 1, "residual": 0.0}

        variants = {"loop": lambda: pagerank_loop(A, args.damping, args.tol, args.cap, symmetric),
                    "call": lambda: A.pagerank(args.damping, args.tol, args.cap, symmetric=symmetric), "product": products}
        if args.only:
            variants = {args.only: variants[args.only]}
        times, infos, outs = {k: [] for k in variants}, {}, {}
        for rep in range(args.reps + 1):
            for key, fn in variants.items():
                ms, (out, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                infos[key], outs[key] = info, out
                if key == "call":
                    iters["n"] = info["iterations"]
        for key in variants:
            med, info = statistics.median(times[key]), infos[key]
            l1 = float((outs["call"] - outs["loop"]).abs().sum().item()) if key == "call" and "loop" in outs else None
            print(json.dumps({"tool": "bench_pagerank", "graph": name, "rows": A.rows, "nnz": A.nnz, "spmv_path": path, "variant": key, "ms": round(med, 3),
                              "ms_min": round(min(times[key]), 3), "ms_max": round(max(times[key]), 3),
                              "ms_per_iteration": round(med / max(info["iterations"], 1), 4), "iterations": info["iterations"], "products": info["products"],
                              "host_waits": info["host_waits"], "residual": info["residual"], "l1_to_loop": l1,
                              "epilogue_model_bytes": 40 * A.rows, "damping": args.damping, "tol": args.tol, "cap": args.cap, "reps": args.reps,
                              "small": args.small}), flush=True)
        A.close()
        del A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
