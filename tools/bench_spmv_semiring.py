#!/usr/bin/env python3
"""g4s_spmv_semiring (min-plus, max-plus, or-and) against g4s_spmv (plus-times, beta = 0) on one handle per matrix, in one process, timed in alternating
rounds, on every SpMV path: rmat = configs[1] (blocked), lap7 = the 431³ stencil and banded = the banded 10M matrix (diagonal), fe = the 207 K-row assembled
FE matrix (block-row), banded_stream = the banded matrix forced onto the row-streaming path. One JSON line per (matrix, semiring, accumulate):
  ms        one product (HIP events over rounds of ≈ 0.1 s, until every variant has --window seconds)
  plus_ms   one g4s_spmv(A, x, y, 1, 0) in the same rounds
  ratio     ms / plus_ms
Usage: python tools/bench_spmv_semiring.py [--matrices rmat,lap7,banded,fe,banded_stream] [--small] [--window 0.5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_spmm import fe_matrix, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="rmat,lap7,banded,fe,banded_stream")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per variant")
    args = ap.parse_args()
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.matrices.split(","):
        if name == "fe":
            A = fe_matrix(host, args.small)
        elif name == "banded_stream":
            B = build_matrix("banded", host, args.small)
            A = host.CSR(B.rowptr, B.colids, B.values, B.rows, B.cols, spmv_flags=capi.SPMV_STREAM)
        else:
            A = build_matrix(name, host, args.small)
        info = A.info()
        x = host.synth_vector(7, A.cols)
        y = torch.empty(A.rows, dtype=torch.float64, device="cuda")
        y0 = host.synth_vector(8, A.rows)
        variants = {"plus_times": lambda: A.spmv(x, y)}
        for sr in ("min_plus", "max_plus", "or_and"):
            variants[sr] = (lambda sr=sr: A.spmv_semiring(x, y, semiring=sr))
            variants[sr + "+acc"] = (lambda sr=sr: A.spmv_semiring(x, y, semiring=sr, accumulate=True))   # (y grows stale: the time does not depend on it)
        y.copy_(y0)
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        t1 = max(max(timed(fn, 1) for fn in variants.values()), 1e-3)
        calls = max(1, int(100.0 / t1))
        tot = {k: [0.0, 0] for k in variants}
        t_end = time.perf_counter() + 2 * args.window * len(variants) + 60.0
        while min(v[0] for v in tot.values()) < 1e3 * args.window and time.perf_counter() < t_end:
            for key, fn in variants.items():
                tot[key][0] += timed(fn, calls)
                tot[key][1] += calls
        ms = {k: v[0] / v[1] for k, v in tot.items()}
        for key in variants:
            if key == "plus_times":
                continue
            sr, acc = key.split("+")[0], key.endswith("+acc")
            print(json.dumps({"tool": "bench_spmv_semiring", "matrix": name, "rows": A.rows, "cols": A.cols, "nnz": A.nnz, "spmv_path": info["spmv_path"],
                              "semiring": sr, "accumulate": acc, "ms": round(ms[key], 5), "plus_ms": round(ms["plus_times"], 5),
                              "ratio": round(ms[key] / ms["plus_times"], 4), "calls": tot[key][1], "small": args.small}), flush=True)
        A.close()
        del A, x, y, y0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
