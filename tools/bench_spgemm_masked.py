#!/usr/bin/env python3
"""Measurements of g4s_spgemm_masked and g4s_triangle_count (profiles/spgemm_masked.txt).

  --case rmat18 | config2     C⟨A⟩ = A ⊗ A against the only way to get these values without the mask: the one-call g4s_spgemm_csr_i32_f64 on the
                              same A followed by the selection of the mask's entries (a sorted-key search on the device), both parts timed. The two
                              ways alternate inside one process, both warmed, median of three rounds with the spread. plus-times and min-plus, values
                              and pattern-only. (The full product's kernels are the same files in this build and in the commit before the masked
                              product existed, so one library serves both sides.)
  --case tri20 | tri_config1  triangles of the symmetrised R-MAT scale 20 / of configs[1]'s matrix symmetrised: time, products per second, class counts,
                              the share of the byte model 4·products + 12·nnz(L) + 8·nnz(L) (pattern-only) over the call's wall time — a model, not
                              HBM traffic: B's rows are re-read from L2 / MALL. The count is cross-checked against runs with class boundaries moved
                              by the environment switches, on tri20 against scipy, and on tri_config1 the full product A·A is attempted once to
                              record its status.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4s_amd import capi, host  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def select(c, mask):
    """values of the full product c at the mask's entries (identity handling left out: the timing is the point)"""
    n = c.cols
    rows = lambda m: torch.repeat_interleave(torch.arange(m.rows, device="cuda"), torch.diff(m.rowptr).long())
    ckey = rows(c) * n + c.colids.long()
    mkey = rows(mask) * n + mask.colids.long()
    pos = torch.searchsorted(ckey, mkey).clamp_(max=max(c.nnz - 1, 0))
    hit = ckey[pos] == mkey
    return torch.where(hit, c.values[pos], torch.zeros((), dtype=torch.float64, device="cuda")), hit


def compare(name, A, rounds=3):
    flop = host.get_flop(A, A)
    for semiring in ("plus_times", "min_plus"):
        full, sel, mv, mp = [], [], [], []
        info = None
        for r in range(rounds + 1):                                # round 0 warms both
            t, c = timed(lambda: host.HashSpGEMM(A, A, semiring=semiring))
            ts, (want, hit) = timed(lambda: select(c, A))
            cnnz = c.nnz
            del c
            tm, (m, info) = timed(lambda: host.spgemm_masked(A, A, A, semiring=semiring, return_info=True))
            tp, _ = timed(lambda: host.spgemm_masked(A, A, A, semiring=semiring, pattern_only=True))
            if r == 0:
                diff = float((m.values[hit] - want[hit]).abs().max().item()) if bool(hit.any()) else 0.0
            else:
                full.append(t); sel.append(ts); mv.append(tm); mp.append(tp)
            del m, want, hit
        print(json.dumps({"case": name, "semiring": semiring, "rows": A.rows, "nnz": A.nnz, "products": flop, "nnz_full_product": cnnz,
                          "full_product": spread(full), "selection": spread(sel), "masked_values": spread(mv), "masked_pattern_only": spread(mp),
                          "max_abs_diff_vs_selection": diff, "info": info}), flush=True)


def symmetrise(A):
    n = A.rows
    r = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.diff(A.rowptr).long())
    c = A.colids.long()
    keep = r != c
    r, c = r[keep], c[keep]
    keys = torch.unique(torch.cat([r * n + c, c * n + r]))
    del r, c
    rows = keys // n
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    del rows
    colids = (keys % n).int()
    return host.CSR(rowptr.int(), colids, torch.ones(colids.numel(), dtype=torch.float64, device="cuda"), n, n)


def triangles(name, G, with_scipy):
    times = []
    for r in range(4):
        t, (count, info) = timed(lambda: G.triangle_count(return_info=True))
        if r:
            times.append(t)
    t_med = statistics.median(times)
    lnnz, products = info["mask_nnz"], info["products"]
    model = 4 * products + 12 * lnnz + 8 * lnnz
    out = {"case": name, "vertices": G.rows, "edges": G.nnz // 2, "triangles": count, "time": spread(times), "products": products,
           "products_per_s": round(products / (t_med * 1e-3), 0), "byte_model_GBps_over_wall_time": round(model / (t_med * 1e-3) / 1e9, 1), "info": info}
    checks = {}
    for switch in ({"G4S_MASKED_WAVE_FLOP": "0"}, {"G4S_MASKED_LDS_LARGE": "0", "G4S_MASKED_LDS_SMALL": "0"}, {"G4S_MASKED_SPLIT_FLOP": "100000"}):
        os.environ.update(switch)
        t, (c2, i2) = timed(lambda: G.triangle_count(return_info=True))
        for k in switch:
            del os.environ[k]
        checks[",".join(f"{k}={v}" for k, v in switch.items())] = {"triangles": c2, "ms": round(t, 3), "info": i2}
        assert c2 == count, (switch, c2, count)
    out["forced_class_cuts"] = checks
    if with_scipy:
        import scipy.sparse as sp
        rp, ci, va = G.to_host()
        L = sp.tril(sp.csr_matrix((va, ci, rp), shape=(G.rows, G.rows)), k=-1).tocsr()
        t0 = time.perf_counter()
        want = int(round((L @ L).multiply(L).sum()))
        out["scipy"] = {"triangles": want, "seconds": round(time.perf_counter() - t0, 1)}
        assert want == count, (want, count)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["rmat18", "config2", "tri20", "tri_config1"])
    ap.add_argument("--small", action="store_true", help="a fraction of the size, to try the tool out")
    a = ap.parse_args()
    if a.case == "rmat18":
        s = 18 if not a.small else 13
        compare("rmat18_ef16", host.rmat_csr(1 << s, s, 16 << s, 20240522))
    elif a.case == "config2":
        s = 21 if not a.small else 14
        compare("configs[2]_rmat21_ef3", host.rmat_csr(1 << s, s, 3 << s, 20240522))
    elif a.case == "tri20":
        s = 20 if not a.small else 14
        triangles("rmat20_ef3_symmetrised", symmetrise(host.rmat_csr(1 << s, s, 3 << s, 20240522)), with_scipy=True)
    else:
        n, s, e = (10_000_000, 24, 100_000_000) if not a.small else (200_000, 18, 2_000_000)
        A = host.rmat_csr(n, s, e, 20240521)
        try:
            c = host.HashSpGEMM(A, A)
            print(json.dumps({"case": "configs[1]_full_product", "status": 0, "nnz": c.nnz}), flush=True)
            del c
        except capi.G4SError as err:
            print(json.dumps({"case": "configs[1]_full_product", "status": err.status, "message": str(err)}), flush=True)
        capi.check(capi.load().g4s_trim())
        G = symmetrise(A)
        del A
        triangles("configs[1]_symmetrised", G, with_scipy=False)


if __name__ == "__main__":
    main()
