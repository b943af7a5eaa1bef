#!/usr/bin/env python3
"""g4s_strongly_connected_components against what a caller could do before, per graph: rmat = configs[1] as given (directed), rmat20 = the directed R-MAT
of scale 20 (edge factor 8) as given, dag_grid = the 1000 × 1000 grid with every edge stored one way only (right and down): acyclic, every vertex is
trimmed, 1999 dependent peel steps — the all-trim worst case. Variants, alternating in every round:
  scc        the call on device pointers with the transpose given (built once, outside the timed region; its time is reported as transpose_ms)
  scc_build  the call with trowptr / tcolids NULL: it builds the transpose itself
  bfs2       a FLOOR for any host loop over the calls that existed before: only the giant component, by two g4s_bfs calls from the call's pivot — on A and
             on the transposed handle — plus one torch compare of the two level vectors (handles created outside the timed region: create_ms)
  scipy      scipy.sparse.csgraph.connected_components(connection="strong") on the host, the copy of the pattern from the device and of the labels back
             included (skipped above --scipy-max entries)
One JSON line per variant: ms (median), ms_min, ms_max over --reps timed rounds after one untimed round, the g4s_scc_info fields, and `equal`: the labels
against scipy's, made canonical (bfs2: its mask against labels == the pivot's label).
Usage: python tools/bench_scc.py [--graphs rmat,rmat20,dag_grid] [--small] [--reps 3] [--no-bfs] [--no-scipy]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kcore import wall  # noqa: E402


def build(name, host, small):
    """(rowptr, colids, n) of a directed pattern on the device"""
    import torch
    from bench import build_matrix
    if name == "rmat":
        A = build_matrix("rmat", host, small)
        return A.rowptr, A.colids, A.rows
    if name == "rmat20":
        scale = 20 if not small else 14
        A = host.rmat_csr(1 << scale, scale, 8 << scale, 20240522)
        return A.rowptr, A.colids, A.rows
    if name == "dag_grid":
        side = 1000 if not small else 100
        v = torch.arange(side * side, dtype=torch.int32, device="cuda").reshape(side, side)
        row = torch.cat([v[:, :-1].flatten(), v[:-1].flatten()])
        col = torch.cat([v[:, 1:].flatten(), v[1:].flatten()])
        rp, ci, _ = host.csr_from_coo(row, col, None, side * side, side * side, dup="first")
        return rp, ci, side * side
    raise SystemExit(f"unknown graph {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="rmat,rmat20,dag_grid")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-bfs", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-max", type=int, default=200_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from g4s_amd import capi, host
    import scc_ref
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        rp, ci, n = build(name, host, args.small)
        nnz = int(ci.numel())
        transpose_ms, (trp, tci, _) = wall(lambda: host.csr_transpose(rp, ci, None, n, n))
        variants = {"scc": lambda: host.strongly_connected_components((rp, ci), transpose=(trp, tci), return_info=True),
                    "scc_build": lambda: host.strongly_connected_components((rp, ci), return_info=True)}
        labels0, info0 = variants["scc"]()
        setup = {"transpose_ms": round(transpose_ms, 3)}
        if not args.no_bfs and info0["pivot"] >= 0:
            ones = torch.ones(nnz, dtype=torch.float64, device="cuda")
            A, T = host.CSR(rp, ci, ones, n, n), host.CSR(trp, tci, ones, n, n)
            setup["create_ms"] = round(wall(lambda: (A.handle, T.handle))[0], 3)
            pivot = info0["pivot"]

            def bfs2():
                fwd, fi = A.bfs([pivot], direction="push")
                bwd, bi = T.bfs([pivot], direction="push")
                return (fwd >= 0) & (bwd >= 0), {"host_waits": fi["host_waits"] + bi["host_waits"], "iterations": fi["iterations"] + bi["iterations"]}
            variants["bfs2"] = bfs2
        if not args.no_scipy and nnz <= args.scipy_max:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import connected_components

            def on_host():
                rp_h, ci_h = rp.cpu().numpy(), ci.cpu().numpy()
                M = sp.csr_matrix((np.ones(nnz, np.int8), ci_h, rp_h), shape=(n, n))
                k, comp = connected_components(M, directed=True, connection="strong")
                return torch.from_numpy(comp).cuda(), {"components": int(k)}
            variants["scipy"] = on_host
        times, infos, outs = {k: [] for k in variants}, {}, {}
        for rep in range(args.reps + 1):
            for key, fn in variants.items():
                ms, (out, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                infos[key], outs[key] = info, out
        want = torch.from_numpy(scc_ref.canonical(outs["scipy"].cpu().numpy())).cuda() if "scipy" in outs else outs["scc"]
        base = {"tool": "bench_scc", "graph": name, "rows": n, "nnz": nnz, "reps": args.reps, "small": args.small}
        for key in variants:
            med = statistics.median(times[key])
            equal = torch.equal(outs[key], want == want[info0["pivot"]]) if key == "bfs2" else True if key == "scipy" else torch.equal(outs[key], want)
            line = dict(base, variant=key, ms=round(med, 3), ms_min=round(min(times[key]), 3), ms_max=round(max(times[key]), 3), **infos[key], equal=bool(equal))
            if key in ("scc", "bfs2"):
                line["setup"] = setup
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
