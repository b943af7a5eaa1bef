#!/usr/bin/env python3
"""g4s_kcore against what a caller could do before, per graph: lap5 = the pattern of configs[0] (1000 × 1000 5-point grid), rmat20_sym = the symmetrised
R-MAT of scale 20 (edge factor 8), rmat_sym = configs[1] symmetrised. Variants, alternating in one process:
  kcore     g4s_kcore on device pointers with `round`;   kcore_core   the same without `round`
  loop      the host loop a user writes over a plan built once (its creation is reported apart): deg = A·alive by g4s_spmv on the pattern without its
            diagonal (values 1.0), then alive &= deg > k in torch, one or two host reads per round
  networkx  networkx.core_number on the host, once, where the graph has at most --networkx-max stored entries (CPU baseline; building the graph is not timed)
One JSON line per variant: ms (median), ms_min, ms_max over --reps timed rounds after one untimed round, the g4s_kcore_info fields (the loop: rounds,
levels, host reads), gentries_per_s (stored entries / median time) and `equal` (core numbers compared with the loop's, or the call's, with ==).
Usage: python tools/bench_kcore.py [--graphs lap5,rmat20_sym,rmat_sym] [--small] [--reps 3] [--no-loop] [--no-networkx]"""
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


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def build(name, host, small):
    """(rowptr, colids, n) of a symmetric pattern with ascending rows"""
    from bench import build_matrix
    from bench_components import symmetrise
    if name == "lap5":
        A = build_matrix("lap5", host, small)
        return A.rowptr, A.colids, A.rows
    if name == "rmat_sym":
        A = build_matrix("rmat", host, small)
        return (*symmetrise(A.rowptr, A.colids, A.rows), A.rows)
    if name == "rmat20_sym":
        scale = 20 if not small else 14
        A = host.rmat_csr(1 << scale, scale, 8 << scale, 20240522)
        return (*symmetrise(A.rowptr, A.colids, A.rows), A.rows)
    raise SystemExit(f"unknown graph {name}")


def spmv_loop(Z):
    """Peeling by products: Z holds the pattern without its diagonal, values 1.0."""
    import torch
    n = Z.rows
    alive = torch.ones(n, dtype=torch.float64, device="cuda")
    deg = torch.empty(n, dtype=torch.float64, device="cuda")
    core = torch.zeros(n, dtype=torch.int32, device="cuda")
    k = rounds = levels = reads = 0
    fresh = True                                                      # no vertex has left at this k yet
    while True:
        Z.spmv(alive, deg)
        live = alive > 0
        low = live & (deg <= k)
        reads += 1
        if bool(low.any()):
            core[low] = k
            alive[low] = 0.0
            rounds += 1
            levels += fresh
            fresh = False
            continue
        reads += 1
        if not bool(live.any()):
            break
        k = int(deg[live].min())
        fresh = True
    return core, {"rounds": rounds, "levels": levels, "host_waits": reads, "products": rounds + levels + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="lap5,rmat20_sym,rmat_sym")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-networkx", action="store_true")
    ap.add_argument("--networkx-max", type=int, default=6_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        rp, ci, n = build(name, host, args.small)
        nnz = int(ci.numel())
        torch.cuda.synchronize()

        def with_round():
            core, _, info = host.kcore((rp, ci), return_round=True, return_info=True)
            return core, info
        variants = {"kcore": with_round, "kcore_core": lambda: host.kcore((rp, ci), return_info=True)}
        setup = None
        if not args.no_loop:
            Z = host.csr_select(host.CSR(rp, ci, torch.ones(nnz, dtype=torch.float64, device="cuda"), n, n), "offdiag")
            t_create, _ = wall(lambda: Z.handle)
            setup = {"create_ms": round(t_create, 3)}
            variants["loop"] = lambda: spmv_loop(Z)
        times, infos, outs = {k: [] for k in variants}, {}, {}
        for rep in range(args.reps + 1):
            for key, fn in variants.items():
                ms, (out, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                infos[key], outs[key] = info, out
        ref = outs.get("loop", outs["kcore"])
        base = {"tool": "bench_kcore", "graph": name, "rows": n, "nnz": nnz, "reps": args.reps, "small": args.small}
        for key in variants:
            med = statistics.median(times[key])
            line = dict(base, variant=key, ms=round(med, 3), ms_min=round(min(times[key]), 3), ms_max=round(max(times[key]), 3), **infos[key],
                        gentries_per_s=round(nnz / (med * 1e-3) / 1e9, 3), equal=bool(torch.equal(outs[key], ref)))
            if key == "loop":
                line["loop_setup"] = setup
            print(json.dumps(line), flush=True)
        if not args.no_networkx and nnz <= args.networkx_max:
            rp_h, ci_h = rp.cpu().numpy(), ci.cpu().numpy()
            import networkx as nx
            rows = np.repeat(np.arange(n), np.diff(rp_h))
            G = nx.Graph()
            G.add_nodes_from(range(n))
            G.add_edges_from(zip(rows[rows < ci_h].tolist(), ci_h[rows < ci_h].tolist()))
            t0 = time.perf_counter()
            c = nx.core_number(G)
            ms = 1e3 * (time.perf_counter() - t0)
            want = np.fromiter((c[v] for v in range(n)), np.int32, n)
            print(json.dumps(dict(base, variant="networkx", ms=round(ms, 1), degeneracy=int(want.max()), equal=bool(np.array_equal(want, ref.cpu().numpy())))),
                  flush=True)
        if not args.no_loop:
            Z.close()
            del Z
        del rp, ci, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
