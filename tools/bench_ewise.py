#!/usr/bin/env python3
"""g4s_csr_ewise_* / g4s_csr_select_* per phase, against scipy on the host, on four cases:
  rmat_sym      the symmetrise of configs[1] (10M R-MAT, directed): transpose, then A ∪ Aᵀ under plus (max costs the same; scipy's maximum drops what is <= 0)
  rmat20_sym    the same for R-MAT scale 20, edge factor 8
  rmat20_union  the union (plus) of two independent R-MAT-20s
  lap7_tril     TRIL (k = 0) on the 431³ 7-point stencil
In one process, --reps rounds after one untimed round. One JSON line per case: ms per phase (median; transpose where there is one, symbolic, numeric),
the entry counts, the g4s_ewise_info fields, achieved bytes/s per phase over the ALGORITHMIC bytes (a model, not a measurement: the symbolic pass reads
4 B per input entry and 2 × 4 B of rowptr per row and writes 4 B of crpt per row; the numeric pass reads 12 B per input entry — 4 B when no values
are read — and writes 12 B per output entry), and scipy's time for the same operation on the host (A + A.T, A + B, sp.tril(A); the copies
are not timed) with `equal`: the two patterns agree and the values agree bit for bit.
Usage: python tools/bench_ewise.py [--cases rmat_sym,rmat20_sym,rmat20_union,lap7_tril] [--small] [--reps 3] [--no-scipy]"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="rmat_sym,rmat20_sym,rmat20_union,lap7_tril")
    ap.add_argument("--small", action="store_true", help="small matrices (a quick check, not the benchmark sizes)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_matrix
    from g4s_amd import capi, host
    lib = capi.load()
    capi.check(lib.g4s_warm_up())
    q, dp = host._ptr_nn, capi.DEVICE_POINTERS

    for name in args.cases.split(","):
        scale = 14 if args.small else 20
        if name == "rmat_sym":
            A = build_matrix("rmat", host, args.small)
        elif name in ("rmat20_sym", "rmat20_union"):
            A = host.rmat_csr(1 << scale, scale, 8 << scale, 20240522)
        elif name == "lap7_tril":
            s = 60 if args.small else 431
            A = host.laplacian_csr(7, s, s, s)
        else:
            raise SystemExit(f"unknown case {name}")
        B = host.rmat_csr(1 << scale, scale, 8 << scale, 20240523) if name == "rmat20_union" else None
        select = name == "lap7_tril"
        combine = "plus"
        rows, cols = A.rows, A.cols
        times = {"transpose": [], "symbolic": [], "numeric": []}
        info, out = capi.EwiseInfo(), None
        for rep in range(args.reps + 1):
            if B is None and not select:
                ms, T = wall(A.transpose)
                if rep:
                    times["transpose"].append(ms)
            else:
                T = B
            crp = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
            cnnz = C.c_int64(0)
            if select:
                sym = lambda: capi.check(lib.g4s_csr_select_symbolic(capi.SELECT_TRIL, 0, 0.0, rows, cols, q(A.rowptr), q(A.colids), q(A.values), q(crp),
                                                                      C.byref(cnnz), dp, host._stream()))
            else:
                sym = lambda: capi.check(lib.g4s_csr_ewise_symbolic(capi.EWISE_UNION, rows, cols, q(A.rowptr), q(A.colids), q(T.rowptr), q(T.colids), q(crp),
                                                                     C.byref(cnnz), dp, C.byref(info), host._stream()))
            ms, _ = wall(sym)
            if rep:
                times["symbolic"].append(ms)
            cci = torch.empty(cnnz.value, dtype=torch.int32, device="cuda")
            cva = torch.empty(cnnz.value, dtype=torch.float64, device="cuda")
            if select:
                num = lambda: capi.check(lib.g4s_csr_select_numeric(capi.SELECT_TRIL, 0, 0.0, rows, cols, q(A.rowptr), q(A.colids), q(A.values), q(crp), q(cci),
                                                                     q(cva), dp, host._stream()))
            else:
                num = lambda: capi.check(lib.g4s_csr_ewise_numeric(capi.EWISE_UNION, host.COMBINERS[combine], rows, cols, q(A.rowptr), q(A.colids), q(A.values),
                                                                    q(T.rowptr), q(T.colids), q(T.values), q(crp), q(cci), q(cva), dp, host._stream()))
            ms, _ = wall(num)
            if rep:
                times["numeric"].append(ms)
            out = (crp, cci, cva)
            if rep < args.reps:
                del crp, cci, cva, T
        n_in = A.nnz + (0 if select else T.nnz)
        n_out = int(out[1].numel())
        med = {k: statistics.median(v) for k, v in times.items() if v}
        sym_bytes = 4 * n_in + 12 * rows * (1 if select else 2) - (4 * rows if not select else 0)
        num_bytes = 12 * n_in + 12 * n_out
        line = {"tool": "bench_ewise", "case": name, "rows": rows, "cols": cols, "nnz_in": n_in, "nnz_out": n_out, "reps": args.reps, "small": args.small,
                "ms": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in times.items() if v},
                "symbolic_gbytes_per_s": round(sym_bytes / (med["symbolic"] * 1e-3) / 1e9, 1), "numeric_gbytes_per_s": round(num_bytes / (med["numeric"] * 1e-3) / 1e9, 1)}
        if not select:
            line.update({k: getattr(info, k) for k, _ in capi.EwiseInfo._fields_ if k != "reserved"})
        if not args.no_scipy:
            import scipy.sparse as sp
            S = sp.csr_matrix((A.values.cpu().numpy(), A.colids.cpu().numpy(), A.rowptr.cpu().numpy()), shape=(rows, cols))
            Sb = None if B is None else sp.csr_matrix((B.values.cpu().numpy(), B.colids.cpu().numpy(), B.rowptr.cpu().numpy()), shape=(rows, cols))
            t0 = time.perf_counter()
            if select:
                W = sp.tril(S, 0, format="csr")
            elif Sb is not None:
                W = (S + Sb).tocsr()
            else:
                W = (S + S.T).tocsr()
            line["scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            W.sort_indices()
            got = sp.csr_matrix((out[2].cpu().numpy(), out[1].cpu().numpy(), out[0].cpu().numpy()), shape=(rows, cols))
            # scipy drops sums equal to zero; scipy_nnz shows whether that happened
            same_pattern = W.nnz == got.nnz and np.array_equal(W.indptr, got.indptr) and np.array_equal(W.indices, got.indices)
            line["scipy_nnz"] = int(W.nnz)
            line["equal"] = bool(same_pattern and np.array_equal(W.data.view(np.int64), got.data.view(np.int64)))
        print(json.dumps(line), flush=True)
        del A, B, T, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
