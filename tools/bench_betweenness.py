#!/usr/bin/env python3
"""g4s_betweenness from 4 sources (as the GAP benchmark's BC kernel uses) on grid = the 5-point pattern of a 300 × 300 grid — the sub-grid of configs[0]'s
1000 × 1000 on which the path counts stay finite (C(598, 299) ≈ 2^594; the full grid reaches about 2^1994 and returns G4S_ERR_OVERFLOW) — and
rmat = configs[1] (10M R-MAT, 100M edges) symmetrised, weights 1. Per graph, the median wall time of the call after betweenness_reserve over --reps
rounds behind one untimed round, sources · nnz / s, and what the call did (levels, host waits, σ maximum). Where the graph is small enough
(--host-nnz-max entries) networkx's betweenness_centrality_subset on the host is timed once on the same sources and its largest relative difference
reported; scipy has no betweenness kernel. Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_betweenness.py`.
Usage: python tools/bench_betweenness.py [--graphs grid,rmat] [--small] [--reps 3] [--sources 4] [--host-nnz-max 2000000]"""
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


def symmetrised(host, G):
    """G with both directions of every entry, duplicates and self-loops dropped, weights 1."""
    import torch
    n = G.rows
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (G.rowptr[1:] - G.rowptr[:-1]).long())
    cols = G.colids.long()
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    keys = torch.unique(torch.cat([rows * n + cols, cols * n + rows]))
    del rows, cols
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return host.CSR(rowptr.to(torch.int32), (keys % n).to(torch.int32), torch.ones(keys.numel(), dtype=torch.float64, device="cuda"), n, n)


def networkx_subset(A, sources):
    import networkx as nx
    import numpy as np
    rp, ci, _ = A.to_host()
    G = nx.DiGraph()
    G.add_nodes_from(range(A.rows))
    G.add_edges_from(zip(np.repeat(np.arange(A.rows), np.diff(rp)).tolist(), ci.tolist()))
    t0 = time.perf_counter()
    total = np.zeros(A.rows)
    nodes = list(range(A.rows))
    for s in sources:
        b = nx.betweenness_centrality_subset(G, [s], nodes, normalized=False)
        total += np.fromiter((b[v] for v in nodes), dtype=np.float64, count=A.rows)
    return 1e3 * (time.perf_counter() - t0), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="grid,rmat")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--host-nnz-max", type=int, default=2_000_000, help="largest graph the networkx comparator is run on")
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        if name == "grid":
            s = 300 if not args.small else 60
            A = symmetrised(host, host.laplacian_csr(5, s, s))
        elif name == "rmat":
            A = symmetrised(host, build_matrix("rmat", host, args.small))
        else:
            raise SystemExit(f"unknown graph {name}")
        torch.cuda.synchronize()
        deg = (A.rowptr[1:] - A.rowptr[:-1]).cpu().numpy()
        candidates = np.flatnonzero(deg > 0)
        sources = np.random.default_rng(20240521).choice(candidates, size=args.sources, replace=False).tolist()
        A.betweenness_reserve()
        out = torch.empty(A.rows, dtype=torch.float64, device="cuda")
        times, info = [], None
        for rep in range(args.reps + 1):
            ms, (_, info) = wall(lambda: A.betweenness(sources, out=out))
            if rep:
                times.append(ms)
        med = statistics.median(times)
        rec = {"tool": "bench_betweenness", "graph": name, "rows": A.rows, "nnz": A.nnz, "sources": sources, "ms": round(med, 3), "ms_min": round(min(times), 3),
               "ms_max": round(max(times), 3), "sources_nnz_per_s": round(len(sources) * A.nnz / (med * 1e-3), 1), "max_degree": int(deg.max()),
               "launches_model": int(2 * info["levels"]), "us_per_level": round(1e3 * med / max(info["levels"], 1), 3), "reps": args.reps, "small": args.small}
        rec.update(info)
        if A.nnz <= args.host_nnz_max:
            host_ms, want = networkx_subset(A, sources)
            got = out.cpu().numpy()
            nz = want > 0
            rec.update({"networkx_ms": round(host_ms, 1), "networkx_sources_nnz_per_s": round(len(sources) * A.nnz / (host_ms * 1e-3), 1),
                        "max_rel_diff_to_networkx": float((np.abs(got - want)[nz] / want[nz]).max()) if nz.any() else 0.0})
        print(json.dumps(rec), flush=True)
        A.close()
        del A, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
