#!/usr/bin/env python3
"""g4s_spmm against k g4s_spmv calls on the same handle, on the matrices bench.py builds (rmat = configs[1], lap7 = the 431³ stencil, banded) and an
assembled FE matrix (block-row path). One JSON line per (matrix, k, layout):
  spmm_ms         one g4s_spmm of k vectors (HIP events, after a warm-up, over a window of at least --window seconds)
  spmv_loop_ms    k g4s_spmv calls over the contiguous columns of a column-major copy of X, timed in the same process, alternating with the SpMM
  ratio           spmm_ms / spmv_loop_ms
  gev_per_s       nnz·k / spmm time, GEdges·vectors/s
  algorithmic_bytes, hbm_share   12·nnz + 4·(rows+1) + 8·k·cols + 8·k·rows (beta = 0: Y is not read), and that over the time as a share of 8 TB/s
  max_rel_err     against the oracle's SpMV per column on a seeded sample of rows (|err| / Σ|a·x|)
A point whose X, Y and their column-major copies do not fit the free device memory is skipped, and its line says so.
Usage: python tools/bench_spmm.py [--matrices rmat,lap7,banded,fe] [--ks 1,2,4,8,16,32] [--small] [--window 0.5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fe_matrix(host, small):
    from tests.helpers import assemble_csr, hex_mesh, spd_blocks
    e = 12 if small else 40
    ien, idmap, nno, neq = hex_mesh(e, e, e)
    rp, ci, va = assemble_csr(ien, idmap, spd_blocks(len(ien), 24, 3), neq)
    return host.CSR.from_host(rp, ci, va, neq, neq)


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def sample_error(oracle, A, rowptr_h, Xc, Y, rows_sample):
    """max |Y − oracle| / Σ|a·x| over the sampled rows, every column (the oracle runs on the sub-matrix of those rows)."""
    import torch
    r = np.sort(rows_sample)
    lens = rowptr_h[r + 1] - rowptr_h[r]
    sub_rp = np.zeros(len(r) + 1, np.int32)
    sub_rp[1:] = np.cumsum(lens)
    idx = np.concatenate([np.arange(rowptr_h[i], rowptr_h[i + 1]) for i in r]) if sub_rp[-1] else np.zeros(0, np.int64)
    it = torch.from_numpy(idx).cuda()
    ci, va = A.colids[it].cpu().numpy(), A.values[it].cpu().numpy()
    got = Y[torch.from_numpy(r).cuda()].cpu().numpy()
    worst = 0.0
    for j in range(Xc.shape[0]):
        x = Xc[j].cpu().numpy()
        want = oracle.spmv(sub_rp, ci, va, x)
        _, asum = oracle.spmv_ld(sub_rp, ci, va, x)
        worst = max(worst, float(np.max(np.abs(got[:, j] - want) / np.maximum(asum, 1e-300))))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="rmat,lap7,banded,fe")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per variant and point")
    args = ap.parse_args()
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    from tests import oracle_lib
    oracle = oracle_lib.load()
    capi.check(capi.load().g4s_warm_up())
    ks = [int(k) for k in args.ks.split(",")]
    for name in args.matrices.split(","):
        A = fe_matrix(host, args.small) if name == "fe" else build_matrix(name, host, args.small)
        info = A.info()
        rowptr_h = A.rowptr.cpu().numpy()
        sample = np.random.default_rng(20240521).choice(A.rows, size=min(A.rows, 2000), replace=False)
        points = [(k, "row") for k in ks] + ([(8, "col")] if 8 in ks else [])
        for k, layout in points:
            line = {"tool": "bench_spmm", "matrix": name, "rows": A.rows, "cols": A.cols, "nnz": A.nnz, "spmv_path": info["spmv_path"], "k": k,
                    "layout": layout, "small": args.small}
            need = 2 * 8 * k * (A.rows + A.cols) + (1 << 30)
            free = torch.cuda.mem_get_info()[0]
            if need > free:
                line["skipped"] = f"needs {need / 1e9:.1f} GB for X, Y and their column-major copies, {free / 1e9:.1f} GB free"
                print(json.dumps(line), flush=True)
                continue
            Xc = host.synth_vector(7, A.cols * k).view(k, A.cols)        # column j contiguous: what the k-call loop reads
            Yc = torch.empty(k, A.rows, dtype=torch.float64, device="cuda")
            if layout == "row":
                X = Xc.t().contiguous()
                Y = torch.empty(A.rows, k, dtype=torch.float64, device="cuda")
            else:
                X, Y = Xc.t(), Yc.t()                                    # the column-major views themselves

            def spmm():
                A.spmm(X, Y)

            def loop():
                for j in range(k):
                    A.spmv(Xc[j], Yc[j])
            spmm()                                                       # reserves the workspace
            loop()
            torch.cuda.synchronize()
            t1 = max(timed(spmm, 1), timed(loop, 1), 1e-3)               # ms of one call: calls per round ≈ 0.1 s
            calls = max(1, int(100.0 / t1))
            tot = {"spmm": [0.0, 0], "loop": [0.0, 0]}
            t_end = time.perf_counter() + 2 * args.window + 30.0
            while (min(tot["spmm"][0], tot["loop"][0]) < 1e3 * args.window) and time.perf_counter() < t_end:
                for key, fn in (("spmm", spmm), ("loop", loop)):
                    tot[key][0] += timed(fn, calls)
                    tot[key][1] += calls
            ms = {key: v[0] / v[1] for key, v in tot.items()}
            alg = 12 * A.nnz + 4 * (A.rows + 1) + 8 * k * A.cols + 8 * k * A.rows
            line.update({"spmm_ms": round(ms["spmm"], 5), "spmv_loop_ms": round(ms["loop"], 5), "ratio": round(ms["spmm"] / ms["loop"], 4),
                         "gev_per_s": round(A.nnz * k / (ms["spmm"] * 1e-3) / 1e9, 3), "algorithmic_bytes": alg,
                         "hbm_share": round(alg / (ms["spmm"] * 1e-3) / 8e12, 4), "calls": {"spmm": tot["spmm"][1], "spmv_loop": tot["loop"][1]},
                         "max_rel_err": sample_error(oracle, A, rowptr_h, Xc, Y, sample)})
            print(json.dumps(line), flush=True)
            del X, Y, Xc, Yc
            torch.cuda.empty_cache()
        A.close()
        del A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
