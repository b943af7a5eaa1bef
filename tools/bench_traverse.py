#!/usr/bin/env python3
"""g4s_sssp / g4s_bfs against the host loops of INTEGRATION.md, on rmat = configs[1] (10M R-MAT, 98.7M edges, weights |a|·0.95 + 0.05, source = the
vertex of largest out-degree) and lap5 = the pattern of configs[0] (1000 × 1000 5-point grid, weights U[0.05, 1), corner source). Per (graph,
algorithm), in one process and alternating the variants round by round (--reps rounds after one untimed round):
  loop   the comparator: spmv_semiring_transpose + clone + equal (SSSP), the or-and loop (BFS) — unchanged code of the library, one host round trip per step
  auto   the library's direction rule;  push / pull   forced
  auto@a auto with G4S_TRAVERSE_ALPHA=a (--alphas): the sweep behind the default switch point
One JSON line per variant: ms (median), ms_min, ms_max, steps, push_steps, pull_steps, host_waits, edges_relaxed, gedges_per_s (edges_relaxed / median time);
every variant's result is compared with the loop's (`equal`).
Usage: python tools/bench_traverse.py [--graphs rmat,lap5] [--small] [--reps 3] [--alphas 4,64,256]"""
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


def sssp_loop(A, src):
    import torch
    d = torch.full((A.rows,), float("inf"), dtype=torch.float64, device="cuda")
    d[src] = 0.0
    steps = 0
    while True:
        prev = d.clone()
        A.spmv_semiring_transpose(prev, d, semiring="min_plus", accumulate=True)
        steps += 1
        if torch.equal(d, prev):
            break
    return d, {"iterations": steps, "push_steps": 0, "pull_steps": steps, "host_waits": steps, "edges_relaxed": steps * A.nnz}


def bfs_loop(A, src):
    import torch
    frontier = torch.zeros(A.rows, dtype=torch.float64, device="cuda")
    frontier[src] = 1.0
    visited, level, depth = frontier.clone(), torch.full((A.rows,), -1, dtype=torch.int32, device="cuda"), 0
    level[src] = 0
    while bool(frontier.any()):
        depth += 1
        frontier = A.spmv_semiring_transpose(frontier, semiring="or_and") * (1.0 - visited)
        level[frontier != 0] = depth
        visited = torch.maximum(visited, frontier)
    return level, {"iterations": depth, "push_steps": 0, "pull_steps": depth, "host_waits": depth, "edges_relaxed": depth * A.nnz}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="rmat,lap5")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alphas", default="", help="comma-separated values of G4S_TRAVERSE_ALPHA to run auto with, beside the default")
    args = ap.parse_args()
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    alphas = [a for a in args.alphas.split(",") if a]
    for name in args.graphs.split(","):
        A = build_matrix(name, host, args.small)
        if name == "rmat":
            A.values.abs_().mul_(0.95).add_(0.05)
            src = int(torch.argmax(A.rowptr[1:] - A.rowptr[:-1]).item())
        else:
            A.values.copy_(torch.from_numpy(__import__("numpy").random.default_rng(17).uniform(0.05, 1.0, A.nnz)).cuda())
            src = 0
        torch.cuda.synchronize()
        A.traverse_reserve()
        for algo, loop, call in (("sssp", sssp_loop, A.sssp), ("bfs", bfs_loop, A.bfs)):
            def auto_at(a):
                def run():
                    os.environ["G4S_TRAVERSE_ALPHA"] = a
                    try:
                        return call([src])
                    finally:
                        del os.environ["G4S_TRAVERSE_ALPHA"]
                return run
            variants = {"loop": lambda: loop(A, src), "auto": lambda: call([src]), "push": lambda: call([src], direction="push"),
                        "pull": lambda: call([src], direction="pull")}
            variants.update({f"auto@{a}": auto_at(a) for a in alphas})
            ref = None
            times, infos, equal = {k: [] for k in variants}, {}, {}
            for rep in range(args.reps + 1):
                for key, fn in variants.items():
                    ms, (out, info) = wall(fn)
                    if rep:
                        times[key].append(ms)
                    infos[key] = info
                    if key == "loop":
                        ref = out
                    equal[key] = bool(torch.equal(out, ref))
            for key in variants:
                med, info = statistics.median(times[key]), infos[key]
                print(json.dumps({"tool": "bench_traverse", "graph": name, "rows": A.rows, "nnz": A.nnz, "source": src, "algo": algo, "variant": key,
                                  "ms": round(med, 3), "ms_min": round(min(times[key]), 3), "ms_max": round(max(times[key]), 3),
                                  "steps": info["iterations"], "push_steps": info["push_steps"], "pull_steps": info["pull_steps"],
                                  "host_waits": info["host_waits"], "edges_relaxed": info["edges_relaxed"],
                                  "gedges_per_s": round(info["edges_relaxed"] / (med * 1e-3) / 1e9, 3), "equal": equal[key], "reps": args.reps,
                                  "small": args.small}), flush=True)
        A.close()
        del A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
