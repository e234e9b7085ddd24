#!/usr/bin/env python3
"""Mixed-precision CG against the fp64 solve, whole solves to 1e-10.

    python tools/cg_mixed_bench.py [--sizes 1024,4096] [--pairs 3]

Per size (sigma 0.2374, m0 -0.06: configs 2 and 3 of BASELINE.md): one context,
the fp64 and the mixed solve through sm_cg_dev alternating in pairs (after one
warm-up solve of each, which also allocates the fp32 buffers). One JSON line
per size: wall time, iterations and us per iteration of each mode, the reliable
updates, the fp64 solve's run-to-run spread (max - min over its repeats, as a
fraction of the median) and the ratio of the medians, with the build id.
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
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--m0", type=float, default=-0.06)
    ap.add_argument("--sigma", type=float, default=0.2374)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100000, help="cut the solves short (profiler runs)")
    a = ap.parse_args()
    import torch
    import schwingermodel_amd as sm
    vp = ctypes.c_void_p
    for N in (int(s) for s in a.sizes.split(",")):
        L = sm.Lattice(N, N)
        V = L.V
        s = torch.cuda.Stream()
        torch.cuda.set_stream(s)
        sm.check(sm.lib.sm_set_stream(L.ctx, vp(s.cuda_stream)))
        U = torch.empty(4 * V, dtype=torch.float64)
        p = torch.empty(4 * V, dtype=torch.float64)
        Un, pn = U.numpy(), p.numpy()
        sm.lib.sm_fill_gauge(4321, a.sigma, N, 0, N, 0, N, Un.ctypes.data, Un[2 * V:].ctypes.data)
        sm.lib.sm_fill_spinor(91011, N, 0, N, 0, N, pn.ctypes.data, pn[2 * V:].ctypes.data)
        dU, dp = U.cuda(), p.cuda()
        x = torch.empty_like(dp)
        sm.check(sm.lib.sm_upload_gauge_dev(L.ctx, vp(dU.data_ptr())))
        res = sm.CGResult()

        def solve(mode):
            L.cg_precision(mode)
            torch.cuda.synchronize()
            t = time.perf_counter()
            sm.check(sm.lib.sm_cg_dev(L.ctx, vp(dp.data_ptr()), vp(x.data_ptr()), a.m0, a.tol, a.max_iter,
                                      ctypes.byref(res)))
            torch.cuda.synchronize()
            return time.perf_counter() - t, res.iterations, res.converged, res.residual / res.phi_norm

        out = {"double": [], "mixed": []}
        for mode in out:
            solve(mode)  # warm-up
        info = None
        for _ in range(a.pairs):
            for mode in out:
                out[mode].append(solve(mode))
                if mode == "mixed":
                    info = L.last_cg_mixed
        rec = {"N": N, "build_id": sm.lib.sm_build_id().decode(), "tol": a.tol, "pairs": a.pairs}
        for mode, runs in out.items():
            walls = [r[0] for r in runs]
            med = statistics.median(walls)
            rec[mode] = {"solve_ms": [round(w * 1e3, 3) for w in walls], "median_ms": round(med * 1e3, 3),
                         "iterations": runs[-1][1], "converged": runs[-1][2], "relres": runs[-1][3],
                         "us_per_iteration": round(med * 1e6 / max(runs[-1][1], 1), 2),
                         "spread": round((max(walls) - min(walls)) / med, 4)}
        rec["mixed"].update(reliable_updates=info.reliable_updates, inner_iterations=info.inner_iterations,
                            fp64_iterations=info.fp64_iterations, fell_back=info.fell_back)
        rec["time_ratio_double_over_mixed"] = round(rec["double"]["median_ms"] / rec["mixed"]["median_ms"], 4)
        print(json.dumps(rec), flush=True)
        L.close()


if __name__ == "__main__":
    main()
