#!/usr/bin/env python3
"""g4s_ktruss against what a caller could do before, per graph: rmat16_sym / rmat18_sym = the symmetrised R-MAT of scale 16 / 18 (edge factor 16),
trigrid = the 1000 × 1000 grid with one diagonal per cell. Variants, alternating in one process:
  ktruss        g4s_ktruss on device pointers with `round` and `support`;   ktruss_truss   the same with the truss numbers alone
  loop          the host loop of INTEGRATION.md, level by level to the same decomposition: supports by spgemm_masked(G, G, G, pattern_only=True) on
                the remaining graph, csr_select("ge", k − 2) on them, the graph cut down to the survivors by an intersect that keeps its values (the
                index of each entry in the input, so that the truss numbers can be written back); when nothing goes, the survivors are the k-truss and
                k jumps to the smallest support + 3. One product, one select and one intersect per round, each with its host reads.
One JSON line per variant: ms (median), ms_min, ms_max over --reps timed rounds after one untimed round (the loop: --loop-reps), the g4s_ktruss_info
fields (the loop: products, levels), gentries_per_s (stored entries / median time) and `equal` (truss numbers compared with the loop's with ==; the
comparison is made on the untimed round, before any timing is kept).
Usage: python tools/bench_ktruss.py [--graphs rmat16_sym,rmat18_sym,trigrid] [--small] [--reps 3] [--loop-reps 3] [--no-loop]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kcore import wall  # noqa: E402


def build(name, host, small):
    """(rowptr, colids, n) of a symmetric pattern with ascending rows, int32 device tensors"""
    import numpy as np
    import torch
    from bench_components import symmetrise
    if name in ("rmat16_sym", "rmat18_sym"):
        scale = int(name[4:6]) - (4 if small else 0)
        A = host.rmat_csr(1 << scale, scale, 16 << scale, 20240613)
        return (*symmetrise(A.rowptr, A.colids, A.rows), A.rows)
    if name == "trigrid":
        side = 1000 if not small else 100
        v = np.arange(side * side, dtype=np.int64).reshape(side, side)
        a = np.concatenate([v[:, :-1].ravel(), v[:-1].ravel(), v[:-1, :-1].ravel()])
        b = np.concatenate([v[:, 1:].ravel(), v[1:].ravel(), v[1:, 1:].ravel()])
        n = side * side
        keys = np.sort(np.concatenate([a * n + b, b * n + a]))
        rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(keys // n, minlength=n), out=rp[1:])
        return torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy((keys % n).astype(np.int32)).cuda(), n
    raise SystemExit(f"unknown graph {name}")


def product_loop(host, rp, ci, n):
    """The truss numbers per stored entry by repeated masked products (see the head of the file)."""
    import torch
    nnz = int(ci.numel())
    truss = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    cur = host.csr_select(host.CSR(rp, ci, torch.arange(nnz, dtype=torch.float64, device="cuda"), n, n), "offdiag")
    truss[cur.values.long()] = 2
    k, products, levels, rounds = 3, 0, 0, 0
    while cur.nnz > 0:
        sup = host.spgemm_masked(cur, cur, cur, pattern_only=True)
        products += 1
        keep = host.csr_select(sup, "ge", thr=float(k - 2))
        if keep.nnz == cur.nnz:                                       # nothing goes: cur is the (smallest support + 2)-truss
            top = int(sup.values.min().item()) + 2
            truss[cur.values.long()] = top
            k = top + 1
            levels += 1
            continue
        rounds += 1
        cur = host.csr_ewise(cur, keep, "intersect", "first")
    return truss, {"products": products, "levels": levels, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="rmat16_sym,rmat18_sym,trigrid")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        rp, ci, n = build(name, host, args.small)
        nnz = int(ci.numel())
        torch.cuda.synchronize()

        def full():
            t, _, _, info = host.ktruss((rp, ci), return_round=True, return_support=True, return_info=True)
            return t, info
        variants = {"ktruss": full, "ktruss_truss": lambda: host.ktruss((rp, ci), return_info=True)}
        if not args.no_loop:
            variants["loop"] = lambda: product_loop(host, rp, ci, n)
        reps = {key: args.loop_reps if key == "loop" else args.reps for key in variants}
        times, infos, outs = {k: [] for k in variants}, {}, {}
        equal = {}
        for rep in range(max(reps.values()) + 1):
            for key, fn in variants.items():
                if rep > reps[key]:
                    continue
                ms, (out, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                else:                                                 # the untimed round: both sides must agree before a time is kept
                    infos[key], outs[key] = info, out
            if rep == 0:
                ref = outs.get("loop", outs["ktruss"])
                equal = {key: bool(torch.equal(outs[key], ref)) for key in variants}
                if not all(equal.values()):
                    print(json.dumps({"tool": "bench_ktruss", "graph": name, "error": "the variants disagree", "equal": equal}), flush=True)
                    break
        else:
            base = {"tool": "bench_ktruss", "graph": name, "rows": n, "nnz": nnz, "small": args.small}
            for key in variants:
                med = statistics.median(times[key])
                print(json.dumps(dict(base, variant=key, reps=reps[key], ms=round(med, 3), ms_min=round(min(times[key]), 3), ms_max=round(max(times[key]), 3),
                                      **infos[key], gentries_per_s=round(nnz / (med * 1e-3) / 1e9, 4), equal=equal[key])), flush=True)
        del rp, ci, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
