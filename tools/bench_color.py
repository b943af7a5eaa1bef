#!/usr/bin/env python3
"""g4s_color against what a caller could do before, per graph: lap5 = the pattern of configs[0] (1000 × 1000 5-point grid), rmat20_sym = the symmetrised
R-MAT of scale 20 (edge factor 8), rmat_sym = configs[1] symmetrised — the graphs of tools/bench_kcore.py. Orders: hash (key = NULL), largest_first
(the flag), smallest_last (key = g4s_kcore's round, computed once outside the timed region; its time is reported as kcore_ms). Variants, alternating in
one process:
  color     g4s_color on device pointers with `round`
  loop      the host loop a user writes over a plan built once (its creation is reported apart): rounds of independent sets by g4s_spmv_semiring max-plus
            on a priority vector over the pattern without its diagonal (values 0.0) — every uncoloured vertex above all its uncoloured neighbours takes
            the round's index as its colour — with one host read per round. ONE COLOUR PER ROUND: its colouring is proper but is not the first-fit one,
            so its colours differ from g4s_color's and there are as many as there are rounds; both counts are reported.
  networkx  networkx.greedy_color with the same explicit order on the host, once, where the graph has at most --networkx-max stored entries (CPU baseline;
            building the graph and the order is not timed); `equal` compares its colours with the call's with ==.
One JSON line per variant and order: ms (median), ms_min, ms_max over --reps timed rounds after one untimed round, the g4s_color_info fields (the loop:
colors, rounds, host reads), gentries_per_s (stored entries / median time) and `proper` (no stored off-diagonal entry joins two vertices of one colour).
Usage: python tools/bench_color.py [--graphs lap5,rmat20_sym,rmat_sym] [--orders hash,largest_first,smallest_last] [--small] [--reps 3] [--no-loop] [--no-networkx]"""
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

from bench_kcore import build, wall  # noqa: E402


def fmix32(x):
    """the murmur3 finaliser on an int64 tensor of values in [0, 2^32)"""
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & m
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & m
    return x ^ (x >> 16)


def priority(n, key, seed=0):
    """the order of g4s_color as one float64 per vertex: key · 2^32 + hash + 1, exact below 2^53"""
    import torch
    h = fmix32(torch.arange(n, dtype=torch.int64, device="cuda") ^ seed)
    k = torch.zeros(n, dtype=torch.int64, device="cuda") if key is None else key.to(torch.int64) - int(key.min())
    return ((k << 32) + h + 1).to(torch.float64)


def spmv_loop(Z, prio):
    """Colouring by products: Z holds the pattern without its diagonal, values 0.0; max-plus gives the largest priority among the uncoloured neighbours."""
    import torch
    n = Z.rows
    x = prio.clone()
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    color = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rounds = 0
    while True:
        Z.spmv_semiring(x, y, semiring="max_plus")
        win = x > y                                                   # coloured vertices hold −inf and never win; an isolated vertex gets y = −inf
        color[win] = rounds
        x[win] = float("-inf")
        rounds += 1
        if not bool((x > float("-inf")).any()):
            break
    return color, {"colors": rounds, "rounds": rounds, "host_waits": rounds, "products": rounds}


def proper(rp, ci, color):
    import torch
    n = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rp.device), (rp[1:] - rp[:-1]).to(torch.int64))
    c = ci.to(torch.int64)
    off = rows != c
    return not bool((color[rows[off]] == color[c[off]]).any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="lap5,rmat20_sym,rmat_sym")
    ap.add_argument("--orders", default="hash,largest_first,smallest_last")
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
        kcore_ms, (_, peel) = wall(lambda: host.kcore((rp, ci), return_round=True))
        deg = (rp[1:] - rp[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device="cuda"), deg)
        deg = (deg - torch.bincount(rows[rows == ci.to(torch.int64)], minlength=n)).to(torch.int32)   # without the diagonal: the key of largest-first
        del rows
        Z = None
        setup = None
        if not args.no_loop:
            Z = host.csr_select(host.CSR(rp, ci, torch.zeros(nnz, dtype=torch.float64, device="cuda"), n, n), "offdiag")
            t_create, _ = wall(lambda: Z.handle)
            setup = {"create_ms": round(t_create, 3)}
        G = None
        for how in args.orders.split(","):
            key = {"hash": None, "largest_first": None, "smallest_last": peel}[how]
            loop_key = deg if how == "largest_first" else key

            def call():
                c, _, info = host.color((rp, ci), key=key, largest_first=how == "largest_first", return_round=True, return_info=True)
                return c, info
            variants = {"color": call}
            if Z is not None:
                prio = priority(n, loop_key)
                variants["loop"] = lambda: spmv_loop(Z, prio)
            times, infos, outs = {k: [] for k in variants}, {}, {}
            for rep in range(args.reps + 1):
                for v, fn in variants.items():
                    ms, (out, info) = wall(fn)
                    if rep:
                        times[v].append(ms)
                    infos[v], outs[v] = info, out
            base = {"tool": "bench_color", "graph": name, "order": how, "rows": n, "nnz": nnz, "reps": args.reps, "small": args.small}
            for v in variants:
                med = statistics.median(times[v])
                line = dict(base, variant=v, ms=round(med, 3), ms_min=round(min(times[v]), 3), ms_max=round(max(times[v]), 3), **infos[v],
                            gentries_per_s=round(nnz / (med * 1e-3) / 1e9, 3), proper=proper(rp, ci, outs[v]))
                if v == "loop":
                    line["loop_setup"] = setup
                if v == "color" and how == "smallest_last":
                    line["kcore_ms"] = round(kcore_ms, 3)
                print(json.dumps(line), flush=True)
            if not args.no_networkx and nnz <= args.networkx_max:
                import networkx as nx
                rp_h, ci_h = rp.cpu().numpy(), ci.cpu().numpy()
                r = np.repeat(np.arange(n), np.diff(rp_h))
                if G is None:
                    G = nx.Graph()
                    G.add_nodes_from(range(n))
                    G.add_edges_from(zip(r[r < ci_h].tolist(), ci_h[r < ci_h].tolist()))
                seq = torch.argsort(priority(n, loop_key), descending=True).cpu().tolist()
                t0 = time.perf_counter()
                c = nx.greedy_color(G, strategy=lambda g, colors: seq)
                ms = 1e3 * (time.perf_counter() - t0)
                want = np.fromiter((c[v] for v in range(n)), np.int32, n)
                print(json.dumps(dict(base, variant="networkx", ms=round(ms, 1), colors=int(want.max()) + 1,
                                      equal=bool(np.array_equal(want, outs["color"].cpu().numpy())))), flush=True)
            del outs
        if Z is not None:
            Z.close()
            del Z
        del rp, ci, peel, deg, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
