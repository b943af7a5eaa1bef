#!/usr/bin/env python3
"""g4s_csr_extract_symbolic / _numeric (host.csr_extract: both calls and the output allocation) on an R-MAT graph, beside the only device route a caller
had before — the algebraic one, P_I · A · P_Jᵀ with selection matrices from host.csr_from_coo and two host.HashSpGEMM calls — in one process on one box:
  the input       the R-MAT edge list of tools/bench_coo.py (same generator, same seed): 16 · 2^20 triples on 2^20 vertices, repeats summed, rows ascending
  (a) induced     A[S, S] for a random half S of the vertices, ids ascending: every row leaves the fill in order, nothing is sorted
  (b) permute     A[p, p] for a random permutation p: every row with more than one entry is sorted, in all three classes
  (c) by_degree   A[p, p] for p = the vertices by descending degree (stable)
  (d) rows_only   A[S, :] with J == NULL (baseline: the one product P_S · A)
Each figure is the median (and the min and max) of --reps timed calls after one untimed call, a host clock around work that ends in a device synchronise.
The two results are compared with == on the row pointers, the column ids and the bits of the values (every value of a product is one value of A times
1.0). Where torch can express a case (index_select on a sparse COO tensor) that is timed too. One JSON line on stdout; --out writes the table.
Usage: python tools/bench_extract.py [--scale 20] [--edge-factor 16] [--reps 5] [--small] [--no-torch] [--cases a,b,c,d] [--out profiles/extract.txt]"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_coo import rmat_edges, wall   # noqa: E402  (the same generator and the same clock)


def timed(fn, reps):
    """(median, min, max) in ms of `reps` calls after one untimed call, and the last result; a result is dropped before the next call is made, so that no
    call pays for the memory of the one before"""
    out = wall(fn)[1]
    ms = []
    for _ in range(reps):
        out = None
        t, out = wall(fn)
        ms.append(t)
    return (statistics.median(ms), min(ms), max(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="scale 14 (a quick check, not the benchmark size)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-compare", action="store_true", help="the new call only (for a profiler run)")
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from g4s_amd import capi, host
    if not torch.cuda.is_available():
        raise SystemExit("bench_extract.py needs a GPU: there is nothing to time without one")
    capi.check(capi.load().g4s_warm_up())
    scale = 14 if args.small else args.scale
    n = 1 << scale
    row, col, val = rmat_edges(scale, args.edge_factor << scale, 20240601)
    rp, ci, va = host.csr_from_coo(row, col, val, n, n, dup="plus")
    del row, col, val
    a = host.CSR(rp, ci, va, n, n)
    g = torch.Generator(device="cuda")
    g.manual_seed(20240602)
    i32 = lambda t: t.to(torch.int32).contiguous()
    half = i32(torch.sort(torch.randperm(n, generator=g, device="cuda")[: n // 2]).values)
    perm = i32(torch.randperm(n, generator=g, device="cuda"))
    degree = (a.rowptr[1:] - a.rowptr[:-1]).to(torch.int64)
    by_degree = i32(torch.sort(degree, descending=True, stable=True).indices)
    cases = {"a": ("induced, half the vertices, ascending", half, half), "b": ("permute, random", perm, perm), "c": ("permute, by descending degree", by_degree, by_degree),
             "d": ("rows only, half the vertices, J = NULL", half, None)}
    arange = lambda k: torch.arange(k, dtype=torch.int32, device="cuda")

    def algebraic(I, J):
        pi = host.CSR.from_coo(arange(I.numel()), I, rows=I.numel(), cols=n)            # P_I(p, I[p]) = 1
        c = host.HashSpGEMM(pi, a)
        if J is None:
            return c
        pjt = host.CSR.from_coo(J, arange(J.numel()), rows=n, cols=J.numel())           # P_Jᵀ(J[q], q) = 1
        return host.HashSpGEMM(c, pjt)

    def with_torch(coo, I, J):
        t = coo.index_select(0, I.to(torch.int64))
        return (t if J is None else t.index_select(1, J.to(torch.int64))).coalesce()

    line = {"tool": "bench_extract", "device": f'{torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]} (the runtime reports it as "{torch.cuda.get_device_name(0)}")', "date": datetime.date.today().isoformat(), "scale": scale, "nnz": a.nnz, "reps": args.reps,
            "cases": {}}
    coo = None
    for key in args.cases.split(","):
        name, I, J = cases[key]
        (med, lo, hi), (c, info) = timed(lambda: host.csr_extract(a, I, J, return_info=True), args.reps)
        res = {"name": name, "nnz_c": c.nnz, "extract_ms": [round(x, 3) for x in (med, lo, hi)],
               "info": {k: info[k] for k in ("j_kind", "units", "rows_in_order", "rows_sorted_wave", "rows_sorted_lds", "rows_sorted_radix", "lds_sort_max", "host_waits")}}
        if not args.no_compare:
            (bmed, blo, bhi), b = timed(lambda: algebraic(I, J), args.reps)
            res["algebraic_ms"] = [round(x, 3) for x in (bmed, blo, bhi)]
            res["equal"] = bool(torch.equal(c.rowptr, b.rowptr) and torch.equal(c.colids, b.colids) and torch.equal(c.values.view(torch.int64), b.values.view(torch.int64)))
            res["speedup"] = round(bmed / med, 2)
            res["gap_exceeds_both_spreads"] = bool(bmed - med > max(hi - lo, bhi - blo))
            del b
            if not args.no_torch:
                try:
                    if coo is None:
                        coo = torch.sparse_csr_tensor(a.rowptr.to(torch.int64), a.colids.to(torch.int64), a.values, (n, n)).to_sparse_coo().coalesce()
                    (tmed, tlo, thi), t = timed(lambda: with_torch(coo, I, J), args.reps)
                    res["torch_ms"] = [round(x, 3) for x in (tmed, tlo, thi)]
                    res["torch_nnz_equal"] = bool(t._nnz() == c.nnz)
                    del t
                except Exception as e:   # noqa: BLE001 - torch cannot express the case on this build: say so in the table
                    res["torch_ms"] = None
                    res["torch_error"] = f"{type(e).__name__}: {str(e)[:120]}"
        del c
        line["cases"][key] = res
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/bench_extract.py on {line['device']}, {line['date']}: R-MAT scale {scale}, {a.nnz} entries; median (min … max) ms of {args.reps} calls "
                    f"after one untimed call\n")
            f.write("extract = host.csr_extract (symbolic + numeric + output allocation); algebraic = csr_from_coo selection matrices + HashSpGEMM (two products, one for d)\n\n")
            f.write(f"{'case':44s} {'entries':>10s} {'extract':>28s} {'algebraic':>32s} {'x':>6s} {'==':>6s} {'torch index_select':>30s}\n")
            fmt = lambda v: "-" if not v else f"{v[0]:.3f} ({v[1]:.3f} … {v[2]:.3f})"
            for key, r in line["cases"].items():
                f.write(f"({key}) {r['name']:40s} {r['nnz_c']:10d} {fmt(r['extract_ms']):>28s} {fmt(r.get('algebraic_ms')):>32s} {r.get('speedup', 0):6.2f} "
                        f"{str(r.get('equal', '-')):>6s} {fmt(r.get('torch_ms')):>30s}\n")
            f.write("\n")
            for key, r in line["cases"].items():
                f.write(f"({key}) {r['info']}" + (f"; gap exceeds both spreads: {r['gap_exceeds_both_spreads']}" if "gap_exceeds_both_spreads" in r else "")
                        + (f"; torch: {r['torch_error']}" if "torch_error" in r else "") + "\n")


if __name__ == "__main__":
    main()
