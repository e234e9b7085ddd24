#!/usr/bin/env python3
"""Batched multi-source CG against K sequential sm_cg_dev solves, whole solves to 1e-10.

    python tools/batch_cg_bench.py [--sizes 64,128,256,1024] [--ks 1,2,4,8,16,32,64] [--pairs 3]
                                   [--tiles N] [--precision double|mixed|both] [--out FILE]

Per size (sigma 0.2374, m0 -0.06: configs 2 and 3 of BASELINE.md): one context,
K sources from K distinct sm_fill_spinor seeds. Per K, after one warm-up of
each side, interleaved pairs of
    one sm_cg_batch_dev solve of the K columns, and
    K sequential sm_cg_dev solves of the same columns (the path a caller had
    before the batch).
Per size and K: wall time of each side (median over the pairs), the iterations
of the slowest column, us per iteration (wall / slowest column's iterations)
and per iteration and column (wall / the columns' summed iterations), the
sequential side's run-to-run spread ((max - min) / median) and the ratio of
the medians, sequential over batch. --tiles N sets the test option
batch_tiles (tiles per launch the batch's tile height aims at; tuning runs).
The records go to stdout as JSON lines and, together, to
profiles/cg_batch_<build id>.json (or --out).

--precision mixed runs both sides in mixed precision (sm_cg_batch_precision and
sm_cg_precision = 1). --precision both compares the batch with itself: the
sides are the fp64 batch and the mixed batch of the same build and context
(sm_cg_batch_precision switched between the solves), from --seq-from sites per
side (default 1024) also K sequential mixed sm_cg_dev solves, which is what a
caller there has today. Its records carry time_ratio_fp64_over_mixed, the fp64
side's spread and `credited` (mixed beats fp64 by more than that spread), and
go to profiles/cg_batch_mixed_<build id>.json.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,1024")
    ap.add_argument("--ks", default="1,2,4,8,16,32,64")
    ap.add_argument("--m0", type=float, default=-0.06)
    ap.add_argument("--sigma", type=float, default=0.2374)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--tiles", type=int, default=0, help="test option batch_tiles (0: the library's default)")
    ap.add_argument("--precision", choices=("double", "mixed", "both"), default="double")
    ap.add_argument("--seq-from", type=int, default=1024, help="--precision both: sequential mixed sm_cg_dev side from this N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.tiles:
        os.environ["SM_TEST_OPTS"] = f"batch_tiles={a.tiles}"
    import torch
    import schwingermodel_amd as sm
    vp = ctypes.c_void_p
    build_id = sm.lib.sm_build_id().decode()
    ks = [int(k) for k in a.ks.split(",") if k]
    kmax = max(ks)
    assert kmax <= sm.lib.sm_cg_batch_max()
    records = []
    for N in (int(s) for s in a.sizes.split(",") if s):
        L = sm.Lattice(N, N)
        V = L.V
        U = torch.empty(4 * V, dtype=torch.float64)
        Un = U.numpy()
        sm.lib.sm_fill_gauge(4321, a.sigma, N, 0, N, 0, N, Un.ctypes.data, Un[2 * V:].ctypes.data)
        phi = torch.empty(kmax, 4 * V, dtype=torch.float64)
        pn = phi.numpy()
        for b in range(kmax):
            sm.lib.sm_fill_spinor(91011 + b, N, 0, N, 0, N, pn[b].ctypes.data, pn[b, 2 * V:].ctypes.data)
        dU, dphi = U.cuda(), phi.cuda()
        xb, xs = torch.empty_like(dphi), torch.empty_like(dphi)
        sm.check(sm.lib.sm_upload_gauge_dev(L.ctx, vp(dU.data_ptr())))
        sm.check(sm.lib.sm_synchronize(L.ctx))
        stride = 4 * V * 8
        if a.precision == "mixed":
            sm.check(sm.lib.sm_cg_batch_precision(L.ctx, 1, None))
        if a.precision != "double":
            sm.check(sm.lib.sm_cg_precision(L.ctx, 1, None))

        def batch(K, mode=None):
            res = (sm.CGResult * K)()
            if mode is not None:
                sm.check(sm.lib.sm_cg_batch_precision(L.ctx, mode, None))
            torch.cuda.synchronize()
            t = time.perf_counter()
            sm.check(sm.lib.sm_cg_batch_dev(L.ctx, K, vp(dphi.data_ptr()), vp(xb.data_ptr()), a.m0, a.tol, a.max_iter, res))
            torch.cuda.synchronize()
            return time.perf_counter() - t, [r.iterations for r in res], all(r.converged for r in res)

        def sequential(K):
            res = sm.CGResult()
            its, conv = [], True
            torch.cuda.synchronize()
            t = time.perf_counter()
            for b in range(K):
                sm.check(sm.lib.sm_cg_dev(L.ctx, vp(dphi.data_ptr() + b * stride), vp(xs.data_ptr() + b * stride), a.m0,
                                          a.tol, a.max_iter, ctypes.byref(res)))
                its.append(res.iterations)
                conv = conv and bool(res.converged)
            torch.cuda.synchronize()
            return time.perf_counter() - t, its, conv

        for K in ks:
            sides = {"batch": batch, "sequential": sequential}
            if a.precision == "both":
                sides = {"batch_fp64": lambda K: batch(K, 0), "batch_mixed": lambda K: batch(K, 1)}
                if N >= a.seq_from:
                    sides["sequential_mixed"] = sequential
            out = {name: [] for name in sides}
            for fn in sides.values():
                fn(K)  # warm-up (the first batched solve of a larger K also regrows the workspace)
            for _ in range(a.pairs):
                for name, fn in sides.items():
                    out[name].append(fn(K))
            rec = {"N": N, "K": K, "build_id": build_id, "tol": a.tol, "pairs": a.pairs, "tiles": a.tiles,
                   "precision": a.precision}
            for name, runs in out.items():
                walls = [r[0] for r in runs]
                med = statistics.median(walls)
                its = runs[-1][1]
                rec[name] = {"solve_ms": [round(w * 1e3, 3) for w in walls], "median_ms": round(med * 1e3, 3),
                             "iterations_slowest": max(its), "iterations_sum": sum(its), "converged": runs[-1][2],
                             "us_per_iteration": round(med * 1e6 / max(max(its), 1), 3),
                             "us_per_iteration_per_column": round(med * 1e6 / max(sum(its), 1), 3),
                             "spread": round((max(walls) - min(walls)) / med, 4)}
            if a.precision == "both":
                ratio = rec["batch_fp64"]["median_ms"] / rec["batch_mixed"]["median_ms"]
                rec["time_ratio_fp64_over_mixed"] = round(ratio, 3)
                rec["credited"] = bool(ratio > 1.0 + rec["batch_fp64"]["spread"])
                if "sequential_mixed" in rec:
                    rec["time_ratio_sequential_mixed_over_batch_mixed"] = round(
                        rec["sequential_mixed"]["median_ms"] / rec["batch_mixed"]["median_ms"], 3)
            else:
                rec["time_ratio_sequential_over_batch"] = round(rec["sequential"]["median_ms"] / rec["batch"]["median_ms"], 3)
                rec["x_max_rel_diff"] = float(((xb[:K] - xs[:K]).norm(dim=1) / xs[:K].norm(dim=1)).max())
            print(json.dumps(rec), flush=True)
            records.append(rec)
        L.close()
        del dphi, xb, xs, dU
        torch.cuda.empty_cache()
    stem = "cg_batch_mixed" if a.precision == "both" else "cg_batch"
    path = a.out or os.path.join(REPO, "profiles", f"{stem}_{build_id}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"build_id": build_id, "records": records}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
