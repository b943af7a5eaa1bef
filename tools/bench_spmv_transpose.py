#!/usr/bin/env python3
"""g4s_csr_transpose, g4s_csr_transpose_reserve and the transposed product against the forward one, on the bench's matrices: rmat = configs[1] (10M R-MAT,
98.7M entries, blocked path), lap7 = the 431³ 7-point stencil and banded = the banded 10M matrix (diagonal path). One JSON line per matrix:
  create_ms     g4s_csr_create of A (first use of the handle; for scale)
  transpose_ms  one g4s_csr_transpose with device pointers, values and perm (wall time of the synchronous call, scratch allocation and release included;
                median of --reps after one untimed call)
  frac_8tbs     the bytes model over transpose_ms, as a fraction of 8 TB/s: read 4(rows + 1) + 12·nnz, written 4(cols + 1) + 16·nnz
  reserve_ms    g4s_csr_transpose_reserve on a fresh handle (the transpose and the inner g4s_csr_create; median of --reps handles)
  ax_ms, atx_ms one g4s_spmv and one g4s_spmv_transpose (HIP events over rounds of about 0.1 s, alternating, until each has --window seconds)
Usage: python tools/bench_spmv_transpose.py [--matrices rmat,lap7,banded] [--small] [--reps 3] [--window 0.5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_spmm import timed  # noqa: E402


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="rmat,lap7,banded")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per product")
    args = ap.parse_args()
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    lib = capi.load()
    capi.check(lib.g4s_warm_up())
    for name in args.matrices.split(","):
        A = build_matrix(name, host, args.small)
        torch.cuda.synchronize()
        create_ms = wall(lambda: A.handle)
        info = A.info()
        rows, cols, nnz = A.rows, A.cols, A.nnz
        trp = torch.empty(cols + 1, dtype=torch.int32, device="cuda")
        tci = torch.empty(nnz, dtype=torch.int32, device="cuda")
        tva = torch.empty(nnz, dtype=torch.float64, device="cuda")
        perm = torch.empty(nnz, dtype=torch.int32, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())
        call = lambda: capi.check(lib.g4s_csr_transpose(rows, cols, nnz, P(A.rowptr), P(A.colids), P(A.values), P(trp), P(tci), P(tva), P(perm),
                                                        capi.DEVICE_POINTERS, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        call()
        t_ms = statistics.median(wall(call) for _ in range(args.reps))
        del trp, tci, tva, perm
        torch.cuda.empty_cache()
        bytes_model = 4 * (rows + 1) + 12 * nnz + 4 * (cols + 1) + 16 * nnz
        res = []
        for _ in range(args.reps):
            B = host.CSR(A.rowptr, A.colids, A.values, rows, cols, spmv_flags=A._spmv_flags)
            B.handle
            res.append(wall(B.transpose_reserve))
            B.close()
        reserve_ms = statistics.median(res)
        A.transpose_reserve()
        tinfo = A.transpose_info()
        x = host.synth_vector(7, cols)
        xt = host.synth_vector(8, rows)
        y = torch.empty(rows, dtype=torch.float64, device="cuda")
        yt = torch.empty(cols, dtype=torch.float64, device="cuda")
        variants = {"ax": lambda: A.spmv(x, y), "atx": lambda: A.spmv_transpose(xt, yt)}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        t1 = max(max(timed(fn, 1) for fn in variants.values()), 1e-3)
        calls = max(1, int(100.0 / t1))
        tot = {k: [0.0, 0] for k in variants}
        t_end = time.perf_counter() + 4 * args.window + 60.0
        while min(v[0] for v in tot.values()) < 1e3 * args.window and time.perf_counter() < t_end:
            for key, fn in variants.items():
                tot[key][0] += timed(fn, calls)
                tot[key][1] += calls
        ms = {k: v[0] / v[1] for k, v in tot.items()}
        print(json.dumps({"tool": "bench_spmv_transpose", "matrix": name, "rows": rows, "cols": cols, "nnz": nnz, "spmv_path": info["spmv_path"],
                          "t_spmv_path": tinfo["spmv_path"], "create_ms": round(create_ms, 3), "transpose_ms": round(t_ms, 3),
                          "bytes_model": bytes_model, "frac_8tbs": round(bytes_model / (t_ms * 1e-3) / 8e12, 4), "reserve_ms": round(reserve_ms, 3),
                          "t_plan_bytes": tinfo["plan_bytes"], "ax_ms": round(ms["ax"], 5), "atx_ms": round(ms["atx"], 5),
                          "atx_over_ax": round(ms["atx"] / ms["ax"], 4), "reps": args.reps, "small": args.small}), flush=True)
        A.close()
        del A, x, xt, y, yt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
