#!/usr/bin/env python3
"""g4s_minimum_spanning_forest against scipy on the host, per graph: lap5 = the configs[0] grid (1000 × 1000, 5-point pattern), rmat_sym = configs[1]
symmetrised, rmat20_sym = the symmetrised R-MAT of scale 20 (edge factor 8), path = a path of 4 M vertices with increasing weights (one round whose
hooks form ONE chain of n − 1: the pointer jumping has the most to do). Weights are seeded and symmetric: an integer in [1, 2^20] hashed from the
vertex pair, so every total is exact and scipy, which takes a stored 0 for no edge, sees every edge. Variants, alternating in every round:
  msf       the call on device pointers with the weights
  msf_null  the same pattern with values == NULL (all ties: a spanning forest)
  scipy     scipy.sparse.csgraph.minimum_spanning_tree on the host, the copy of the matrix from the device included (one timed run; skipped above
            --scipy-max entries)
One JSON line per variant: ms (median), ms_min, ms_max over --reps timed rounds after one untimed round, the g4s_msf_info fields, walked_per_round, and
`equal`: edges and total weight against scipy's, labels against g4s_connected_components.
path1k (not in the default list) is the same path with 1000 vertices: the fixed cost of a call against scipy on a graph that small.
Usage: python tools/bench_msf.py [--graphs lap5,rmat_sym,rmat20_sym,path,path1k] [--small] [--reps 3] [--no-scipy]"""
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
    """(rowptr, colids, n) of a symmetric pattern on the device"""
    import torch
    from bench_components import build as build_pattern
    if name in ("path", "path1k"):                                  # path1k: a call whose fixed cost (the launches, the waits) is all there is
        n = 1000 if name == "path1k" else 4_000_000 if not small else 100_000
        i = torch.arange(n - 1, dtype=torch.int32, device="cuda")
        rp, ci, _ = host.csr_from_coo(i, i + 1, None, n, n, dup="first", symmetric=True)
        return rp, ci, n
    rp, ci, n, _ = build_pattern(name, host, small)
    return rp, ci, n


def weights(name, host, rp, ci, n):
    """float64 device tensor: symmetric integer weights in [1, 2^20]; on the path the weight of {i, i + 1} is i + 1"""
    import torch
    row = host.csr_row_indices(rp, int(ci.numel())).long()
    col = ci.long()
    lo, hi = torch.minimum(row, col), torch.maximum(row, col)
    if name in ("path", "path1k"):
        return (lo + 1).double()
    return (((lo * 2654435761 + hi * 40503) >> 7) % (1 << 20) + 1).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="lap5,rmat_sym,rmat20_sym,path")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-max", type=int, default=40_000_000)
    args = ap.parse_args()
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        rp, ci, n = build(name, host, args.small)
        nnz = int(ci.numel())
        w = weights(name, host, rp, ci, n)
        variants = {"msf": lambda: host.minimum_spanning_forest((rp, ci, w), return_labels=True),
                    "msf_null": lambda: host.minimum_spanning_forest((rp, ci), return_labels=True)}
        times, infos, outs = {k: [] for k in variants}, {}, {}
        for rep in range(args.reps + 1):
            for key, fn in variants.items():
                ms, (pos, labels, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                infos[key], outs[key] = info, (pos, labels)
        cc = host.connected_components((rp, ci), symmetric=True)
        scipy_line = None
        if not args.no_scipy and nnz <= args.scipy_max:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import minimum_spanning_tree

            def on_host():
                M = sp.csr_matrix((w.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n, n))
                T = minimum_spanning_tree(M)
                return int(T.nnz), float(T.sum())
            ms, (s_edges, s_weight) = wall(on_host)
            scipy_line = {"variant": "scipy", "ms": round(ms, 3), "edges": s_edges, "weight": s_weight}
        base = {"tool": "bench_msf", "graph": name, "rows": n, "nnz": nnz, "reps": args.reps, "small": args.small}
        for key in variants:
            info, (pos, labels) = infos[key], outs[key]
            equal = torch.equal(labels, cc) and info["edges"] == n - info["components"]
            if scipy_line is not None:
                equal = equal and info["edges"] == scipy_line["edges"] and (key == "msf_null" or info["weight"] == scipy_line["weight"])
            med = statistics.median(times[key])
            line = dict(base, variant=key, ms=round(med, 3), ms_min=round(min(times[key]), 3), ms_max=round(max(times[key]), 3), **info,
                        walked_per_round=round(info["entries_walked"] / max(info["rounds"], 1)), equal=bool(equal))
            if scipy_line is not None:
                line["scipy_over_msf"] = round(scipy_line["ms"] / med, 2)
            print(json.dumps(line), flush=True)
        if scipy_line is not None:
            print(json.dumps(dict(base, **scipy_line)), flush=True)


if __name__ == "__main__":
    main()
