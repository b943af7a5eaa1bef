#!/usr/bin/env python3
"""g4s_connected_components against what a caller could do before, per graph: lap5 = the pattern of configs[0] (1000 × 1000 5-point grid), rmat =
configs[1] as given (10M R-MAT, directed), rmat_sym = its symmetrised pattern, rmat20_sym = R-MAT scale 20, edge factor 8, symmetrised.
In one process, alternating the variants round by round (--reps rounds after one untimed round):
  cc        g4s_connected_components on device pointers, without the flag;   cc_sym   with G4S_CC_SYMMETRIC (symmetric patterns only)
  loop      the comparator: min-plus label propagation l := l ⊕ (Z ⊗ l) ⊕ (Zᵀ ⊗ l) until nothing changes, Z = the pattern with all values 0.0, through
            spmv_semiring + spmv_semiring_transpose (accumulate) — the library's API before this call existed, one host round trip per round. Its
            set-up (the handle's plan and the transpose reserve) is timed once and reported separately as loop_setup.
  scipy     scipy.sparse.csgraph.connected_components(directed=True, connection="weak") on the host, once (CPU baseline; the copy to the host is not timed)
  cc@r/s    (--sweep) G4S_CC_SAMPLE_ROUNDS=r, G4S_CC_NO_SKIP=s, with the flag where the pattern is symmetric
One JSON line per variant: ms (median), ms_min, ms_max, the g4s_cc_info fields, gentries_per_s (stored entries / median time), model_gbytes_per_s under
the byte model below, and `equal`: the labels equal the loop's (and scipy's canonicalised labels equal them too).
Byte model (a model, not a measurement): every stored entry is read once (4 B) and gathers one parent (4 B) in the pass that touches it; per vertex
2 × 4 B of rowptr, and 8 B per compress pass actually run (≈ 1 + rounds) plus 12 B for open and count: bytes = 8·nnz + (20 + 8·(2 + rounds))·n.
Usage: python tools/bench_components.py [--graphs lap5,rmat,rmat_sym,rmat20_sym] [--small] [--reps 3] [--sweep] [--no-scipy] [--no-loop]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def symmetrise(rowptr, colids, n):
    """The pattern of A + Aᵀ as (rowptr, colids) int32 device tensors, rows sorted, duplicates merged."""
    import torch
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), (rowptr[1:] - rowptr[:-1]).to(torch.int64))
    cols = colids.to(torch.int64)
    keys = torch.unique(torch.cat([rows * n + cols, cols * n + rows]), sorted=True)
    del rows, cols
    r = keys // n
    ci = (keys - r * n).to(torch.int32)
    rp = torch.zeros(n + 1, dtype=torch.int64, device=rowptr.device)
    rp[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return rp.to(torch.int32), ci


def build(name, host, small):
    """(rowptr, colids, n, symmetric)"""
    from bench import build_matrix
    if name == "lap5":
        A = build_matrix("lap5", host, small)
        return A.rowptr, A.colids, A.rows, True
    if name in ("rmat", "rmat_sym"):
        A = build_matrix("rmat", host, small)
        if name == "rmat":
            return A.rowptr, A.colids, A.rows, False
        return (*symmetrise(A.rowptr, A.colids, A.rows), A.rows, True)
    if name == "rmat20_sym":
        scale = 20 if not small else 14
        A = host.rmat_csr(1 << scale, scale, 8 << scale, 20240522)
        return (*symmetrise(A.rowptr, A.colids, A.rows), A.rows, True)
    raise SystemExit(f"unknown graph {name}")


def label_loop(Z):
    import torch
    l = torch.arange(Z.rows, dtype=torch.float64, device="cuda")
    rounds = 0
    while True:
        prev = l.clone()
        Z.spmv_semiring(prev, l, semiring="min_plus", accumulate=True)
        Z.spmv_semiring_transpose(prev, l, semiring="min_plus", accumulate=True)
        rounds += 1
        if torch.equal(l, prev):
            break
    return l.to(torch.int32), {"rounds": rounds, "host_waits": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="lap5,rmat,rmat_sym,rmat20_sym")
    ap.add_argument("--small", action="store_true", help="small graphs (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also every G4S_CC_SAMPLE_ROUNDS x G4S_CC_NO_SKIP setting")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from g4s_amd import capi, host
    capi.check(capi.load().g4s_warm_up())
    for name in args.graphs.split(","):
        rp, ci, n, symmetric = build(name, host, args.small)
        nnz = int(ci.numel())
        torch.cuda.synchronize()

        def cc(sym, env=None):
            def run():
                for k, v in (env or {}).items():
                    os.environ[k] = v
                try:
                    return host.connected_components((rp, ci), symmetric=sym, return_info=True)
                finally:
                    for k in (env or {}):
                        del os.environ[k]
            return run
        variants = {"cc": cc(False)}
        if symmetric:
            variants["cc_sym"] = cc(True)
        setup = None
        if not args.no_loop:
            Z = host.CSR(rp, ci, torch.zeros(nnz, dtype=torch.float64, device="cuda"), n, n)
            t_create, _ = wall(lambda: Z.handle)
            t_reserve, _ = wall(Z.transpose_reserve)
            setup = {"create_ms": round(t_create, 3), "transpose_reserve_ms": round(t_reserve, 3)}
            variants["loop"] = lambda: label_loop(Z)
        if args.sweep:
            for r in range(5):
                for s in (0, 1):
                    variants[f"cc@{r}/{s}"] = cc(symmetric, {"G4S_CC_SAMPLE_ROUNDS": str(r), "G4S_CC_NO_SKIP": str(s)})
        times, infos, outs = {k: [] for k in variants}, {}, {}
        for rep in range(args.reps + 1):
            for key, fn in variants.items():
                ms, (out, info) = wall(fn)
                if rep:
                    times[key].append(ms)
                infos[key], outs[key] = info, out
        ref = outs.get("loop", outs["cc"])
        scipy_line = None
        if not args.no_scipy:
            import components_ref
            rp_h, ci_h = rp.cpu().numpy(), ci.cpu().numpy()
            t0 = time.perf_counter()
            want, k = components_ref.scipy_labels(rp_h, ci_h, n)
            scipy_line = {"ms": round(1e3 * (time.perf_counter() - t0), 1), "components": int(k),
                          "equal": bool(np.array_equal(want, ref.cpu().numpy()))}
        base = {"tool": "bench_components", "graph": name, "rows": n, "nnz": nnz, "symmetric": symmetric, "reps": args.reps, "small": args.small}
        for key in variants:
            med, info = statistics.median(times[key]), infos[key]
            line = dict(base, variant=key, ms=round(med, 3), ms_min=round(min(times[key]), 3), ms_max=round(max(times[key]), 3), **info,
                        gentries_per_s=round(nnz / (med * 1e-3) / 1e9, 3), equal=bool(torch.equal(outs[key], ref)))
            if key.startswith("cc"):
                line["model_gbytes_per_s"] = round((8 * nnz + (20 + 8 * (2 + info["sample_rounds"])) * n) / (med * 1e-3) / 1e9, 1)
            if key == "loop":
                line["loop_setup"] = setup
            print(json.dumps(line), flush=True)
        if scipy_line:
            print(json.dumps(dict(base, variant="scipy", **scipy_line)), flush=True)
        if not args.no_loop:
            Z.close()
            del Z
        del rp, ci, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
