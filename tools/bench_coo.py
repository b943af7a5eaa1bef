#!/usr/bin/env python3
"""g4s_csr_from_coo_symbolic / _numeric on a skewed edge list with repeats, beside what a caller could do before, in one process on one box:
  the input       R-MAT (0.57, 0.19, 0.19, 0.05) ids composed bit by bit from torch's generator on the device (fixed seed): 16 · 2^20 triples on 2^20
                  vertices, weights 1 … 8 (integers: every summation order gives the same bits, so the comparison lines can be checked with ==)
  symbolic        the sort, the head flags, the scan and the row pointers (dup = plus)
  numeric         the fill with the fold
  presorted       the symbolic call on the same list in (row, col) order: no pass runs
  transpose_x2    g4s_csr_transpose twice on a CSR of the same entry count (the list under "keep") — what include/g4s.h told callers to do for unsorted
                  rows before; it merges nothing
  torch           torch.sparse_coo_tensor(...).coalesce() followed by to_sparse_csr()
  scipy           coo_matrix(...).tocsr() with sum_duplicates() and sort_indices() on the host (the copies are not timed)
Each line is the median of --reps timed calls after one untimed call, a host clock around work that ends in a device synchronise. The algorithmic bytes
are a model, not a measurement: the key pass reads 8 B and writes 12 B per triple, a sort pass reads 8 B (count) and 12 B (scatter; 8 B in the first pass)
and writes 12 B, the head flags read 8 B and write 4 B, the scan reads and writes 4 B; the fill reads 4 B of perm, 8 B of ids and 8 B of value per
triple and writes 12 B per entry. One JSON line on stdout; --out writes the table.
Usage: python tools/bench_coo.py [--scale 20] [--edge-factor 16] [--reps 5] [--small] [--no-scipy] [--out profiles/coo.txt]"""
import argparse
import ctypes as C
import datetime
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


def median_ms(fn, reps):
    wall(fn)
    return statistics.median(wall(fn)[0] for _ in range(reps))


def rmat_edges(scale, n, seed):
    """n (row, col) pairs on 2^scale vertices, every bit of the two ids drawn from the four quadrants with R-MAT's probabilities."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    row = torch.zeros(n, dtype=torch.int32, device="cuda")
    col = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(scale):
        u = torch.rand(n, generator=g, device="cuda")
        row = row * 2 + (u >= 0.76).to(torch.int32)                     # quadrants c and d
        col = col * 2 + (((u >= 0.57) & (u < 0.76)) | (u >= 0.95)).to(torch.int32)   # quadrants b and d
    val = torch.randint(1, 9, (n,), generator=g, device="cuda").to(torch.float64)
    return row.contiguous(), col.contiguous(), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="scale 14 (a quick check, not the benchmark size)")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-compare", action="store_true", help="the two calls only (for a profiler run)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from g4s_amd import capi, host
    if not torch.cuda.is_available():
        raise SystemExit("bench_coo.py needs a GPU: there is nothing to time without one")
    lib = capi.load()
    capi.check(lib.g4s_warm_up())
    q, dp = host._ptr_nn, capi.DEVICE_POINTERS
    scale = 14 if args.small else args.scale
    rows = cols = 1 << scale
    n = args.edge_factor << scale
    row, col, val = rmat_edges(scale, n, 20240601)
    dup = capi.COMBINE_PLUS

    crp = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    cnnz, info = C.c_int64(0), capi.CooInfo()
    sym = lambda r=row, c=col: capi.check(lib.g4s_csr_from_coo_symbolic(dup, rows, cols, n, q(r), q(c), q(crp), q(perm), C.byref(cnnz), dp, C.byref(info),
                                                                        host._stream()))
    ms = {"symbolic": median_ms(sym, args.reps)}
    inf = {k: getattr(info, k) for k, _ in capi.CooInfo._fields_ if k != "reserved"}
    nout = cnnz.value
    cci = torch.empty(nout, dtype=torch.int32, device="cuda")
    cva = torch.empty(nout, dtype=torch.float64, device="cuda")
    num = lambda: capi.check(lib.g4s_csr_from_coo_numeric(dup, rows, cols, n, q(row), q(col), q(val), q(crp), q(perm), q(cci), q(cva), dp, host._stream()))
    ms["numeric"] = median_ms(num, args.reps)
    got = (crp.cpu().numpy().copy(), cci.cpu().numpy().copy(), cva.cpu().numpy().copy())
    line = {"tool": "bench_coo", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "scale": scale, "triples": n,
            "reps": args.reps, **inf}
    if not args.no_compare:
        p = perm.to(torch.int64)
        srow, scol = row[p].contiguous(), col[p].contiguous()
        ms["presorted"] = median_ms(lambda: sym(srow, scol), args.reps)
        line["presorted_flag"] = info.presorted
        del srow, scol, p
        krp, kci, kva = host.csr_from_coo(row, col, val, rows, cols, dup="keep")
        ms["transpose_x2"] = median_ms(lambda: host.csr_transpose(*host.csr_transpose(krp, kci, kva, rows, cols), cols, rows), args.reps)
        del krp, kci, kva
        idx = torch.stack([row.to(torch.int64), col.to(torch.int64)])

        def with_torch():
            return torch.sparse_coo_tensor(idx, val, (rows, cols)).coalesce().to_sparse_csr()
        ms["torch"] = median_ms(with_torch, args.reps)
        t = with_torch()
        line["torch_equal"] = bool(np.array_equal(t.crow_indices().cpu().numpy(), got[0]) and np.array_equal(t.col_indices().cpu().numpy(), got[1])
                                   and np.array_equal(t.values().cpu().numpy().view(np.int64), got[2].view(np.int64)))
        del t, idx
        if not args.no_scipy:
            import scipy.sparse as sp
            hr, hc, hv = row.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()

            def with_scipy():
                m = sp.coo_matrix((hv, (hr, hc)), shape=(rows, cols)).tocsr()
                m.sum_duplicates()
                m.sort_indices()
                return m
            t0 = time.perf_counter()
            m = with_scipy()
            ms["scipy"] = 1e3 * (time.perf_counter() - t0)
            line["scipy_equal"] = bool(np.array_equal(m.indptr, got[0]) and np.array_equal(m.indices, got[1])
                                       and np.array_equal(m.data.view(np.int64), got[2].view(np.int64)))
    passes = inf["sort_passes"]
    sort_bytes = n * (32 * passes - 4)
    sym_bytes = n * 20 + sort_bytes + n * 12 + n * 8 + 4 * rows
    num_bytes = n * 20 + n * 12 + n * 8 + 12 * nout
    line.update({"ms": {k: round(v, 3) for k, v in ms.items()}, "ns_per_triple": {k: round(1e6 * v / n, 3) for k, v in ms.items()},
                 "symbolic_algorithmic_gbytes_per_s": round(sym_bytes / (ms["symbolic"] * 1e-3) / 1e9, 1),
                 "numeric_algorithmic_gbytes_per_s": round(num_bytes / (ms["numeric"] * 1e-3) / 1e9, 1)})
    if "transpose_x2" in ms:
        line["transpose_x2_over_symbolic_plus_numeric"] = round(ms["transpose_x2"] / (ms["symbolic"] + ms["numeric"]), 2)
    print(json.dumps(line), flush=True)
    if args.out:
        names = {"symbolic": "g4s_csr_from_coo_symbolic (plus)", "numeric": "g4s_csr_from_coo_numeric (plus)", "presorted": "symbolic, input already sorted",
                 "transpose_x2": "g4s_csr_transpose twice (merges nothing)", "torch": "torch coalesce + to_sparse_csr", "scipy": "scipy tocsr + sum_duplicates (host)"}
        with open(args.out, "w") as f:
            f.write(f"tools/bench_coo.py on {line['device']}, {line['date']}: R-MAT scale {scale}, {n} triples -> {nout} entries, longest run {inf['longest_run']}\n")
            f.write(f"key bits {inf['row_bits']} + {inf['col_bits']}, {passes} passes of {inf['digit_bits']} bits, tile {inf['tile_entries']}, host waits {inf['host_waits']};"
                    f" median of {args.reps} calls after one untimed call\n\n")
            f.write(f"{'call':44s} {'ms':>10s} {'ns/triple':>10s}\n")
            for k, v in ms.items():
                f.write(f"{names[k]:44s} {v:10.3f} {1e6 * v / n:10.3f}\n")
            f.write(f"\nalgorithmic GB/s (a model): symbolic {line['symbolic_algorithmic_gbytes_per_s']}, numeric {line['numeric_algorithmic_gbytes_per_s']}\n")
            if "transpose_x2" in ms:
                f.write(f"transpose twice / (symbolic + numeric) = {line['transpose_x2_over_symbolic_plus_numeric']}\n")
            for k in ("torch_equal", "scipy_equal"):
                if k in line:
                    f.write(f"{k}: {line[k]}\n")


if __name__ == "__main__":
    main()
